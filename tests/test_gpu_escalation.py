"""famfinder's escalation past 4096 candidates, end to end: a store of 6010 references in which only ten, of a foreign
clade, are full length, fs-req-full = 1, and sixteen queries of which ten have to widen their candidate list 41 -> 410 ->
4100 -> the whole store before a full-length relative turns up (tests/kmer_big_cases.py: escalation_world;
tests/test_kmer_big_cpu.py checks on the CPU that they must).  Family, alignment and log against the oracle, query by
query; the rounds above 4096 go through the device's big select in one launch each.  And the search stage with
search-kmer-candidates = 4500 on a 6000-reference store of its own."""
import pytest

from sina_amd import pipeline
from tests import kmer_big_cases as kb
from tests import util
from tests.test_gpu_pipeline import _check
from tests.test_gpu_search import _search_stage_case

pytestmark = pytest.mark.gpu

N_ESCALATE = 10          # (test_kmer_big_cpu.py: test_escalation_world_escalates)


def test_famfinder_escalates_through_the_big_select(oracle):
    refs, _, _ = kb.escalation_world()
    qs = kb.escalation_queries()
    cs = util.cseqs_from_refs(refs)
    idx = oracle.Index(cs, k=10)
    st = pipeline.Store(":mem:gpu-escalation", refs)
    try:
        pl = pipeline.Pipeline(st, famfinder=kb.ESC_FF_OPTS)
        big0, l0 = st.big_select_queries(), st.stats()["kmer_launches"]
        pl.run(qs.mask, qs.off, batch=qs.n, inflight=1)
        n_dp, n_copy = _check(oracle, refs, qs, pl, cs, idx, ff=kb.ESC_FF)
        assert n_dp + n_copy == qs.n
        pl.close()
        # the rounds of 4100 and of 6010 candidates, for the queries that must escalate at least
        assert st.big_select_queries() - big0 >= N_ESCALATE
        # ... as launches per round, not per query
        assert 0 < st.stats()["kmer_launches"] - l0 < qs.n
    finally:
        st.close()


def test_search_stage_with_4500_kmer_candidates(oracle):
    """search-kmer-candidates above 4096: the candidates of the comparison are the big select's."""
    _search_stage_case(oracle, 6000, {"search-kmer-candidates": 4500}, dict(kmer_candidates=4500), n_queries=5)
