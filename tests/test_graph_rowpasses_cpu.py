"""tests/graph_rowpass_cases.py on the CPU: every family sits on the edge its name says, the plain build accepts it, none
runs into the refusal of more than 32 768 spill rows, and the launches of tests/test_gpu_graph_rowpasses.py hold every
place the kernel keeps the rows' codes.  (So no case of the GPU test can skip or be refused on the device.)"""
import numpy as np
import pytest

from tests import graph_cases as gc, graph_ref as gr, graph_rowpass_cases as rc


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_case_sits_on_its_edge(case):
    g = case.graph()
    assert 0 < g["n"] <= gc.FIRST_NCAP and len(case.family()) <= 128
    assert case.on_edge()
    for ring in rc.rings_of(case):
        w = case.words(ring)
        assert w["n_spill"] <= gr.MAX_SPILL_ROWS
        assert len(w["z"]) == g["n"] and len(w["pred"]) == len(g["pred"])


def test_launch_groups_hold_every_place_of_the_codes():
    for name, members in rc.GROUPS.items():
        cases = [rc.BY_NAME[m] for m in members]
        sizes = {len(c.family()) for c in cases}
        assert len(sizes) == 1, name      # (one family size: however the launch is cut, the room is the same)
        f = sizes.pop()
        assert {rc.fit(c.graph()["n"], f) for c in cases} == {"two", "one", "global"}, name
    fits = {rc.fit(c.graph()["n"], len(c.family())) for c in rc.CASES}
    assert fits == {"two", "one", "global"}


def test_bound_of_restates_the_column_sums():
    g = rc.BY_NAME["fence-beside-sink"].graph()
    r, c, gmin = rc.bound_of(g, np.float32(64.0) * np.float32(1.0001) * np.float32(2.0))
    assert r[-1] == 0 and c[-1] == 0 and (np.diff(r) <= 0).all() and gmin >= 2
    assert r[10] == r[11] and c[10] == c[11] and r[9] > r[10]      # (rows 10 and 11 share column 10)
