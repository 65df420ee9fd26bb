"""--fs-no-graph with the profile built on the device (sina_hip_align_profiles): what can be checked without a GPU --
the ABI surface, the refusal of a null context, and that the host's option routing is what it was; the profile
kernel's named cases (tests/profile_cases.py) each on the edge it names, and its plain restatement
(tests/profile_ref.py) pinned to the oracle's pseq + base_profile::comp, to the host twin (build_family_profile,
family_graph.cpp) and -- the chain's words -- to dp_plan.h's prep_range (tests/dp_plan_check.cpp --words)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sina_amd import capi, pipeline
from tests import profile_cases as pc, profile_ref as pr, util
from tests.test_graph_cpu import plan_check  # noqa: F401  (the fixture: dp_plan_check under the sanitizers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_symbols_are_exported_and_declared():
    L = capi.load()
    for s in ("sina_hip_align_profiles", "sina_hip_debug_family_profile"):
        assert s in capi.ABI_SYMBOLS
        assert hasattr(L, s), s
    hdr = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+sina_hip_align_profiles\s*\(", code)
    assert re.search(r"\bint\s+sina_hip_debug_family_profile\s*\(", code)
    # the header cites what the entry point restates, like the other entries
    doc = hdr[:hdr.index("int sina_hip_align_profiles")]
    doc = doc[doc.rindex("/*"):]
    assert "src/align.cpp:428-433" in doc and "src/pseq.cpp" in doc and "src/pseq.h:65-113" in doc
    assert L.sina_hip_abi_version() == 5     # (a function was added, no structure changed)


def test_align_profiles_refuses_a_null_context_with_a_message():
    L = capi.load()
    p = capi.AlignParams()
    L.sina_hip_align_params_default(C.byref(p))
    assert L.sina_hip_align_profiles(None, None, None, 0, None, None, C.byref(p), None, None) != 0
    msg = L.sina_hip_last_error()
    assert b"align_profiles" in msg and b"null" in msg
    n = C.c_uint32()
    assert L.sina_hip_debug_family_profile(None, None, 1, -2.0, 1.0, 5.0, 2.0, C.byref(n), None, None, None, 0) != 0
    assert b"debug_family_profile" in L.sina_hip_last_error()
    # the entry point it shares its launch loop with still names itself
    assert L.sina_hip_align_families(None, None, None, 0, None, None, C.byref(p), None, None) != 0
    assert b"align_families" in L.sina_hip_last_error()


def test_host_option_routing_is_unchanged():
    H = pipeline.load_host()
    H.sina_host_reset_options()
    try:
        for v in (b"1", b"0"):
            assert H.sina_host_set_option(b"aligner", b"device-graph", v) == 0
            assert H.sina_host_set_option(b"aligner", b"fs-no-graph", v) == 0
        assert H.sina_host_set_option(b"aligner", b"device-graph", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"fs-no-graph", b"1") == 0     # both at once: still the host build ...
        assert H.sina_host_set_option(b"aligner", b"device-profile", b"1") == 0  # ... until this asks for the device route
        assert H.sina_host_set_option(b"aligner", b"use-subst-matrix", b"1") != 0
        assert H.sina_host_set_option(b"aligner", b"no-such-option", b"1") != 0
    finally:
        H.sina_host_reset_options()


# ---------------------------------------------------------------- the named cases and the plain build

IDS = [c.name for c in pc.CASES]
FUZZ_SEEDS = range(int(os.environ.get("SINA_FUZZ_SEEDS", "12")))


def test_case_names_are_unique_and_the_kernel_numbers_are_the_sources():
    assert len(set(IDS)) == len(IDS)
    src = open(os.path.join(ROOT, "sina_amd", "csrc", "profile_build.hip")).read()
    ctx = open(os.path.join(ROOT, "sina_amd", "csrc", "ctx.h")).read()
    assert re.search(r"constexpr int kPT = %d;" % pc.THREADS, src) and re.search(r"constexpr uint32_t kTileMax = %d;" % pc.TILE_MAX, src)
    assert "c->prof_ncap ? c->prof_ncap : %du;" % pc.FIRST_NCAP in src and "i0 += %d)" % pc.CHUNK in src
    assert "const uint32_t i = i0 + %du * (uint32_t)u + lane;" % pc.LANES in src and pc.CHUNK == 4 * pc.LANES
    assert "constexpr uint32_t kLdsSlack = %d;" % pc.LDS_SLACK in src and "budget = %d * 1024 - kLdsSlack" % (pc.LDS_BYTES // 1024) in src
    assert "sizeof(PMember) == %d" % pc.MEMBER_BYTES in src and "need_n + need_n / 8 + 16" in src and "max_n + max_n / 8 + 16" in src
    assert "(0x346Cu >> (4u * (order - 1u))) & 0xFu" in src and [(0x346C >> 4 * (k - 1)) & 15 for k in (1, 2, 3, 4)] == [12, 6, 4, 3]
    assert re.search(r"constexpr int kFamilyMax = %d;" % pc.FAMILY_MAX, ctx) and 'test_knob("profile_tile")' in src
    # (profile_lds as profile_cases.host_tile adds it up: the full tile for every store a case uses; a forced tile never
    # exceeds what the LDS allows and is never less than 1)
    assert pc.host_tile(12800, 3, 65535) == pc.TILE_MAX and pc.host_tile(800, 128, pc.FIRST_NCAP) == pc.FIRST_NCAP
    assert pc.host_tile(524288, 128, 65535) == (160 * 1024 - 256 - 6 * 16384 - 24 * 128 - 16) // 12 == 5182
    assert pc.host_tile(524288, 128, 65535, 6000) == 5182 and pc.host_tile(800, 1, 4096, 64) == 64 and pc.host_tile(800, 1, 4096, 0) == 4096
    assert pc.grown_ncap(4097) == 4625 and pc.grown_ncap(65000) == 65535
    assert pc.SMALL_TILES == (1, 2, 64, 511, 512, 513)


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_case_sits_on_its_edge(case):
    assert case.on_edge(), case.name
    assert pc.finite(case) and case.build()["n"] <= 65535
    if case.fresh:
        assert len(case.fam) <= 3 and case.tiles == (None,)
    else:
        assert set(pc.SMALL_TILES) | {None} <= set(case.tiles) and case.build()["n"] <= 1100
        assert len(case.fam) <= 8 or (len(case.fam) == 128 and case.name.startswith("count-"))


def test_the_edges_asked_for_are_all_there():
    names = set(IDS)
    assert {"tile-open-on-next-tiles-first-node", "tile-stretch-clamped-to-n0", "tile-member-absent-from-a-whole-tile",
            "tile-member-ended-tiles-ago", "tile-first-base-in-the-third-tile", "tile-cursor-hand-over",
            "tile-beyond-exit-two-chunks-left", "tile-n-equals-t", "tile-n-equals-t-plus-1", "tile-n-equals-2t",
            "tile-n-equals-512", "tile-n-equals-513", "tile-n-equals-1024", "tile-fewer-nodes-than-threads", "tile-of-512-nodes",
            "tile-of-513-nodes", "members-8-one-per-wave"} <= names
    assert {"bitless-first-base", "bitless-run-behind-a-base", "bitless-behind-a-gap", "bitless-run-behind-a-gap",
            "bitless-leading-run", "bitless-behind-a-base", "bitless-walk-back-across-a-tile",
            "bitless-walk-back-across-a-tile-in-a-gap", "bitless-last-base", "bitless-column-0"} <= names
    assert {"rank-one-word", "rank-width-4001", "rank-512-words", "rank-513-words", "rank-bit-0-and-bit-31",
            "rank-last-column-occupied", "rank-column-0-occupied", "rank-column-0-empty"} <= names
    assert {"count-128-same-base", "count-orders-2-3-4", "count-127-gaps-open", "count-128-gaps-extend",
            "count-128-stretches-end-on-one-node"} <= names
    assert {"length-%d" % k for k in (0, 1, 63, 64, 65, 255, 256, 257, 513)} <= names
    assert {"chain-one-node", "chain-one-node-a-base", "chain-two-nodes", "same-reference-twice"} <= names
    assert {"host-%d-nodes" % n for n in (4096, 4097, 6144, 6145, 12288, 12289)} <= names
    assert sum(len(c.fam) == 128 for c in pc.CASES) == 4 and max(c.build()["n"] for c in pc.CASES) == 12289
    # a node needs a base (or is column 0, where every gap is a leading one): no more than F - 1 gaps open on a node
    assert all(int(c.build()["points"][:, 4].max()) // 12 < len(c.fam) for c in pc.CASES)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_families_are_finite_and_within_the_limits(seed):
    case = pc.fuzz_case(seed)
    assert pc.finite(case) and 1 <= len(case.fam) <= pc.FAMILY_MAX and 1 <= case.tiles[0] <= 700
    b = case.build()
    total = b["points"].sum(axis=1)          # (twelve points per member, none for a base without a base bit)
    assert b["n"] <= 65535 and (total > 0).all() and (total <= 12 * len(case.fam)).all()
    assert np.isfinite(case.tables()[0][:, 1:]).all()
    again = pc.fuzz_case(seed)
    assert all((x == y).all() for x, y in zip(case.members, again.members)) and case.tiles == again.tiles


def test_the_fuzz_draws_every_code_order_and_long_absences():
    cases = [pc.fuzz_case(s) for s in range(12)]
    orders = {pr.order_of(m) for c in cases for mb in c.members for m in np.unique(mb >> 24)}
    assert orders == {0, 1, 2, 3, 4}
    assert {len(c.fam) for c in cases} & {1} and max(len(c.fam) for c in cases) > 100
    assert any(max(r1 - r for r, r1, _ in pc.stretches(c.build(), m)) > 100 for c in cases for m in c.members if len(m))
    assert any(c.build()["n"] > 2 * c.tiles[0] for c in cases)


def _cseqs(oracle, members, width):
    return [oracle.Cseq.from_packed("m%d" % i, np.asarray(m, np.uint32), width) for i, m in enumerate(members)]


def _same_as_the_oracle(oracle, b, fam, scores, what):
    """pos, the six shares and every table entry of the plain build against oracle.pseq_build + oracle.profile_comp."""
    o, tab, own = util.profile_oracle_tables(oracle, fam, *scores)
    assert b["n"] == o["n"] and (b["pos"] == o["pos"]).all(), what
    assert (util.f32_bits(pr.shares(b["points"])) == util.f32_bits(np.asarray(o["prof"], np.float32).reshape(-1, 6))).all(), what
    got, gown = pr.table(b["points"], *scores)
    assert np.isposinf(got[:, 0]).all() and (util.f32_bits(got[:, 1:]) == util.f32_bits(tab[:, 1:])).all(), what
    assert (util.f32_bits(gown[1:]) == util.f32_bits(own[1:])).all() and gown[0] == 0, what


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_plain_build_equals_oracle_pseq(oracle, case):
    _same_as_the_oracle(oracle, case.build(), _cseqs(oracle, case.family(), case.width), pc.SCORES, case.name)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_plain_build_equals_oracle_pseq_on_the_fuzz_families(oracle, seed):
    case = pc.fuzz_case(seed)
    _same_as_the_oracle(oracle, case.build(), _cseqs(oracle, case.family(), case.width), pc.SCORES, seed)
    # ... and on the plane fuzz's worlds (their families can hold a column of bases without a base bit alone: NaN there,
    # on both sides -- the bits are compared)
    rng, pick, refs, cs, usable = util.fuzz_world(seed)
    ids = list(rng.permutation(usable)[:int(pick([1, 2, 7, 40, 60]))])
    b = pr.build([refs.seq(int(i)) for i in ids], refs.width)
    _same_as_the_oracle(oracle, b, [cs[int(i)] for i in ids], (-2.0, 1.0, 5.0, 2.0), (seed, len(ids)))


def test_plain_build_equals_the_host_twin():
    """build_family_profile (host/family_graph.cpp), what the aligner's host route hands to sina_hip_align_graphs."""
    groups = pc.by_width() + pc.by_width(fresh=True) + [(None, [pc.fuzz_case(s)]) for s in range(4)]
    for k, (width, cases) in enumerate(groups):
        refs, fams = pc.refset(cases)
        st = pipeline.Store(":mem:profilecases%d" % k, refs)
        try:
            for case, ids in zip(cases, fams):
                pos, tab, own = st.build_profile(ids, *pc.SCORES)
                want, wown = case.tables()
                assert len(pos) == case.build()["n"] and (pos == case.build()["pos"]).all(), case.name
                assert (util.f32_bits(tab) == util.f32_bits(want)).all() and (util.f32_bits(own) == util.f32_bits(wown)).all(), case.name
        finally:
            st.close()


@pytest.mark.parametrize("name", ["chain-one-node", "chain-two-nodes", "tile-cursor-hand-over"])
def test_chain_words_equal_prep_range(plan_check, tmp_path, name):  # noqa: F811
    case = next(c for c in pc.CASES if c.name == name)
    g, w = pr.chain_graph(case.build()["pos"]), case.words()
    n = g["n"]
    assert n == {"chain-one-node": 1, "chain-two-nodes": 2}.get(name, n) and (n <= 2 or n > 300)
    path = str(tmp_path / "chain.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (n, len(g["pred"])))
        for a in (g["pos"], g["mask"], util.f32_bits(g["weight"]), g["pred_off"], g["pred"]):
            f.write(" ".join(str(int(x)) for x in a) + "\n")
    for ring in (1, 4, 8):   # (every row is handed on in registers: the ring does not matter)
        run = subprocess.run([plan_check, "--words", path, str(ring)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert run.returncode == 0, run.stdout[-4000:]
        lines = run.stdout.split("\n")
        assert lines[0] == "sizes %d %d %d" % (w["sizes"][0], w["sizes"][2], w["sizes"][4])
        rows = np.array([ln.split() for ln in lines[1:1 + n]], np.uint32)
        assert (rows[:, 0] == w["rec"][:, 2]).all() and (rows[:, 1] == w["rec"][:, 3]).all(), (name, ring)
        assert (np.array(lines[1 + n:n + n], np.uint32) == w["pred"]).all(), (name, ring)
    assert list(w["sizes"]) == [n, n - 1, 0, 0, n - 1, 0] and (w["rec"][:, 3] == pr.gr.ROW_NONE).all() and (w["rec"][:, 1] == 0).all()
    assert (w["succ_min"] == np.append(case.build()["pos"][1:], 1000000)).all()


def test_abi_has_the_profile_words_entry():
    hdr = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    assert re.search(r"#define SINA_HIP_ABI_VERSION 5\b", hdr)     # (a function was added, no structure changed)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+sina_hip_debug_family_profile_words\s*\(", code)
    assert "sina_hip_debug_family_profile_words" in capi.ABI_SYMBOLS
    L = capi.load()
    assert hasattr(L, "sina_hip_debug_family_profile_words") and L.sina_hip_abi_version() == 5
    n = C.c_uint32()
    assert L.sina_hip_debug_family_profile_words(None, None, 1, C.byref(n), None, None, None, None, 0) != 0
    assert b"debug_family_profile_words" in L.sina_hip_last_error()
