"""CPU side of the wide path: every case of tests/wide_cases.py reaches the edge it is there for (asserted on the
oracle's planes and the plain walk, as tests/test_walk_cpu.py does for walk_cases.py), and the additions to the C ABI,
its Python view and the aligner's options are in place."""
import os
import re

import numpy as np

from sina_amd import capi, pipeline
from tests import util, wide_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sina_hip_align_graphs_any", "sina_hip_debug_mesh_wide", "sina_hip_wide_queries",
               "sina_hip_last_error_is_limit")


def _npred(g):
    return np.diff(g["pred_off"].astype(np.int64))


def test_fan_in_enters_through_a_late_predecessor(oracle):
    c = wc.fan_in()
    g = c.graph
    hub = 1 + wc.FAN_SINGLES
    assert _npred(g).max() == _npred(g)[hub] == 300 > 255
    for variant, _ in wc.variants(c.width, len(c.qmasks[0])):
        rows = list(wc.reference(c.name, 0, variant)[1]["rows"])
        via = rows[rows.index(hub) + 1]
        ordinal = list(g["pred"][g["pred_off"][hub]:g["pred_off"][hub + 1]]).index(via)
        assert via == wc.FAN_VIA and ordinal >= 256, (variant, via, ordinal)


def test_long_chain_stays_above_65535(oracle):
    c = wc.long_chain()
    assert c.graph["n"] == 66000 > 65535 and len(c.qmasks[0]) == 12
    wk = wc.reference(c.name, 0)[1]
    assert wk["end_m"] == wc.CHAIN_END and wk["rows"].min() >= 65536


def test_far_edges_need_more_spill_rows_than_the_fast_kernel_has(oracle):
    c = wc.far_edges()
    g = c.graph
    assert g["n"] <= 65535 and _npred(g).max() <= 255 and len(c.qmasks[0]) == 12
    where = util.row_store_model(g["pred_off"], g["pred"], 4)
    assert int(((where & 0x80000000) != 0).sum()) > 32768
    rows = wc.reference(c.name, 0)[1]["rows"]
    assert (np.abs(np.diff(rows)) == wc.FAR_STEP).any(), rows


def test_long_query_and_long_diagonal(oracle):
    c = wc.long_query()
    assert len(c.qmasks[0]) == 10241 and c.graph["n"] == 40
    wk = wc.reference(c.name, 0)[1]
    assert wk["cutoff_head"] > 0 and wk["cutoff_tail"] > 0 and wk["aligned_bases"] >= 30
    c = wc.long_diagonal()
    n, L = c.graph["n"], len(c.qmasks[0])
    assert L > n > 1024 and L <= 10240
    assert wc.reference(c.name, 0)[1]["stats"]["longest_ins_run"] > 50


def test_tiny_cases(oracle):
    cases = {c.name: c for c in wc.tiny()}
    assert [(c.graph["n"], len(c.qmasks[0])) for c in (cases["tiny-1x1"], cases["tiny-1x5"], cases["tiny-5x1"])] == \
        [(1, 1), (1, 5), (5, 1)]
    late = cases["tiny-late-sources"].graph
    assert list(late["src"]) == [0, 3, 5]
    # some walk ends at a source that is not row 0 or passes a row whose predecessor is one
    assert any(set(wc.reference("tiny-late-sources", qi)[1]["rows"]) & {3, 4, 5, 6} for qi in range(3))
    tie = cases["tiny-end-tie"]
    planes, wk = wc.reference(tie.name, 0)
    last = planes["value"][:, -1]
    snk = int(tie.graph["snk"][0])
    ties = np.flatnonzero(last == last.min())
    assert snk in ties and any(int(m) != snk and m < snk for m in ties)    # a non-sink row ties with the sink, and comes first
    assert wk["end_m"] == snk


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "sina_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert sym in capi.ABI_SYMBOLS
    assert "#define SINA_HIP_ABI_VERSION 5" in header
    for name in ("align_graphs_any", "debug_mesh_wide", "wide_queries"):
        assert callable(getattr(capi.Context, name))


def test_aligner_takes_wide_fallback():
    H = pipeline.load_host()
    try:
        assert H.sina_host_set_option(b"aligner", b"wide-fallback", b"1") == 0
        assert H.sina_host_set_option(b"aligner", b"wide-fallback", b"0") == 0
    finally:
        H.sina_host_reset_options()
