"""The bitmap loop of kmer_count_kernel<false / true> and kmer_count_long_kernel where it fetches its rows
(csrc/kmer_count_tile.inc): the cases of tests/kmer_dense_rows_cases.py -- chunk and padding edges of the number fetch,
the all-zero row against real rows the query does not contain, the skipped waves of the last tile, chunks of a long
query adding to the row -- uploaded with sina_hip_upload_index and compared, every score and every top-`max` exactly,
with tests/kmer_ref.py's plain model, on candidate lists and on score rows (tests/test_gpu_kmer.py's runner).  And
dense_overflow of tests/kmer_cases.py once more: 1023 bitmap numbers, sixteen whole chunks less one."""
import pytest

from tests import kmer_dense_rows_cases as rc
from tests.test_gpu_kmer import _run


@pytest.mark.parametrize("name", list(rc.CASES))
def test_cases_reach_their_edges(name):
    """CPU: every builder's assertions (what is dense, how many bitmap numbers a query has, where the planted
    references sit and what they score, which waves of the last tile are live)."""
    c = rc.case(name)
    assert c.expected and all(len(e["scores"]) == c.n_refs for e in c.expected)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rc.CASES))
def test_kmer_dense_rows(monkeypatch, name):
    _run(rc.case(name), monkeypatch)
