"""Every align entry starts through the one guard (ctx.h, align_call): whatever the call before it counted, an entry that
brings no family to the device leaves sina_hip_staged_identity NULL, a debug entry leaves sina_hip_staged_pair_counts
NULL as well, and the in-place kernels' counters move only for what the entry may count.

The launch is identity_cases' shared_family group -- the smallest one with an ordinary width, the one
test_gpu_identity.py's test_nothing_counted runs -- with a helix map on the store; the graphs entries get its first
query against its family's host-built DAG."""
import numpy as np
import pytest

from sina_amd import capi
from tests import identity_cases as ic, util

pytestmark = pytest.mark.gpu


def _weighted(ctx, width):
    """params and sets of a _wsets call: two vectors of ones (the alignment is the unweighted one), the query takes the second"""
    return ctx.params_wsets(np.ones((2, width), np.float32), assemble=1), np.array([1], np.uint32), 2


def _graphs_wsets(ctx, gb, qmask, qoff):
    p, sets, n = _weighted(ctx, gb.width)
    return ctx.align_graphs_wsets(gb, qmask, qoff, p, sets, n)


# (name, call(ctx, graph batch, qmask, qoff) -> (out, pos) or planes, whether the entry may count pairs): a new entry that
# brings no family to the device is one more row
OTHER_ENTRIES = (
    ("align_graphs", lambda ctx, gb, qmask, qoff: ctx.align_graphs(gb, qmask, qoff, ctx.params(assemble=1)), True),
    ("align_graphs_wsets", _graphs_wsets, True),
    ("align_graphs_any", lambda ctx, gb, qmask, qoff: ctx.align_graphs_any(gb, qmask, qoff, ctx.params(assemble=1)), True),
    ("debug_mesh", lambda ctx, gb, qmask, qoff: ctx.debug_mesh(gb, qmask, ctx.params(assemble=1)), False),
    ("debug_mesh_wide", lambda ctx, gb, qmask, qoff: ctx.debug_mesh_wide(gb, qmask, ctx.params(assemble=1)), False),
)


def test_every_entry_forgets_what_the_call_before_counted(oracle):
    (launch, ref), = ic.group("shared_family")
    want = ic.rows(ref)
    width = launch.width
    helix = np.zeros(width, np.uint32)          # nested: column c with column width - c, where the world has its bases
    for c in range(10, width // 2, 10):
        helix[c], helix[width - c] = width - c, c
    fam, foff = launch.packed_families()
    qmask_all, qoff_all = launch.packed_queries()
    ctx = capi.Context(0)
    try:
        ctx.upload_refs(launch.refs.ab, launch.refs.off.astype(np.uint64), width)
        ctx.upload_pairs(helix)
        ctx.count_pairs(True)
        ctx.count_identity(True)
        gb = ctx.graph_batch([util.graph_dict(util.cseqs_from_refs(launch.refs, launch.fam_ids[0]))], width)
        qmask = launch.qmasks[0]
        qoff = np.array([0, len(qmask)], np.uint64)
        for name, call, may_count_pairs in OTHER_ENTRIES:
            out, _ = ctx.align_families(fam, foff, qmask_all, qoff_all, ctx.params(assemble=1))      # the counting call
            assert (out["status"] == 0).all(), name
            assert (ctx.staged_identity() == want).all() and ctx.staged_pair_counts() is not None, name
            p0, i0 = ctx.pair_inplace_stats(), ctx.identity_inplace_stats()
            got = call(ctx, gb, qmask, qoff)
            rows = ctx.staged_pair_counts()
            p1, i1 = ctx.pair_inplace_stats(), ctx.identity_inplace_stats()
            print(name, "pairs", p0, "->", p1, "identity", i0, "->", i1)
            assert ctx.staged_identity() is None, name
            assert i1 == i0, name
            if not may_count_pairs:
                assert rows is None and p1 == p0, name
                continue
            o, pos = got
            assert o[0]["status"] == 0 and o[0]["assembled"] == 1, name
            assert p1["launches"] - p0["launches"] == 1 and p1["sequences"] - p0["sequences"] == 1, (name, p0, p1)
            n_out = int(o[0]["n_out"])
            assert rows is not None and rows.shape == (1, 6), name
            assert (rows == ctx.pair_counts(pos[:n_out], np.array([0, n_out], np.uint64))).all(), name
    finally:
        ctx.close()
