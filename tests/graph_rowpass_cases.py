"""Families for the passes behind the device DAG build's tile loop (family_graph_kernel steps 6-9, sina_amd/csrc/
graph_build.hip): sink / fence flags, the slot allocation's segments, spill rows numbered across segments, predecessor
entries, the row-skip bound -- and the three places the kernel keeps the rows' codes while it runs them.  Shared by
tests/test_graph_rowpasses_cpu.py (every case sits on the edge it names, the plain build accepts it) and
tests/test_gpu_graph_rowpasses.py (which runs them).  CPU work on hand-built packed arrays, as tests/graph_cases.py.

Where the codes are kept follows from the LDS in front of the occupied-column bitmap, graph_cases.graph_bitmap_off(F)
bytes for a launch whose largest family has F members, 4 bytes a row:
  "two"    rows' codes and the column maxima beside them (8 bytes a row fit): step 9's maxima run beside step 7's walk
  "one"    the codes alone fit: step 9 runs behind step 8, in the codes' place
  "global" not even the codes fit: rec / last in global memory."""
import numpy as np

from tests import graph_cases as gc, graph_ref as gr

A, G, C, U = gc.A, gc.G, gc.C, gc.U
RINGS = (4, 8)            # the slot search is compiled for 4 slots (W <= 4) and for 8
RINGS_MORE = (1, 3, 4, 5, 8)
WIDTH = 10240


def fit(n_rows, max_family):
    room = gc.graph_bitmap_off(max_family)
    return "two" if 8 * n_rows <= room else "one" if 4 * n_rows <= room else "global"


def rows_that_fit(max_family, words):
    """The largest DAG of which `words` words a row fit the tile tables' space."""
    return gc.graph_bitmap_off(max_family) // (4 * words)


def ladder(n):
    """n rows, three members: a chain over all columns, every third column again (edges of 3 rows: LDS slots), and a
    member that jumps (edges of 7, 40, 193 and 300 rows in turn: slots, spill rows, fence rows)."""
    cols = [0]
    for k in range(n):
        nxt = cols[-1] + (7, 40, 193, 300)[k % 4]
        if nxt >= n:
            break
        cols.append(nxt)
    return [gc.mem(range(n)), gc.mem(range(0, n, 3)), gc.mem(cols)]


def disjoint(n_members, each):
    """Members with columns of their own, one after the other: n_members * each rows, a sink at every member's end."""
    return [gc.mem(range(j * each, (j + 1) * each), [(A, G, C, U)[(i + j) % 4] for i in range(each)]) for j in range(n_members)]


def _z(c, ring=4):
    return c.words(ring)["z"]


def _npred(g):
    return np.diff(g["pred_off"].astype(np.int64))


def _cases():
    cs = []

    def add(name, members, edge, **kw):
        cs.append(gc.Case(name, members, edge, width=WIDTH, **kw))

    # ---- 1. rows around the allocator's 16 lanes and its segments of max(256, ceil(N / 16)) rows
    for n in (1, 2, 15, 16, 17):
        add("rows-%d" % n, ladder(n), lambda g, c, n=n: g["n"] == n and gc.slot_segment(n) == 256)
    for n in (256, 257, 512, 513):
        add("rows-%d" % n, ladder(n), lambda g, c, n=n: g["n"] == n and (n % gc.slot_segment(n) == 0) == (n % 2 == 0) and
            (g["n"] + gc.slot_segment(n) - 1) // gc.slot_segment(n) < 16)
    add("rows-4096-16-segments", ladder(4096), lambda g, c: g["n"] == 4096 and gc.slot_segment(4096) == 256 and fit(4096, 3) == "one", big=True)
    add("rows-4097-segments-of-257", ladder(4097), lambda g, c: g["n"] == 4097 and gc.slot_segment(4097) == 257 and fit(4097, 3) == "one", big=True)
    # ---- 2. spill rows at a segment's boundary, numbered in row order across three segments
    add("boundary-spills", [gc.mem(range(600)), gc.mem([250, 300]), gc.mem([254, 256]), gc.mem([100, 256]), gc.mem([255, 256]),
                            gc.mem([500, 520]), gc.mem([511, 512]), gc.mem([3, 9]), gc.mem([300, 310, 515]), gc.mem([520, 530])],
        lambda g, c: g["n"] == 600 and all(gc.spilled(c, 8, r) for r in (100, 250, 254, 500, 310)) and
        c.words(8)["store"][255] == gr.ROW_NONE and c.words(8)["store"][511] == gr.ROW_NONE and      # (only the next row reads them)
        not gc.spilled(c, 8, 3) and not gc.spilled(c, 8, 520) and
        [int(c.words(8)["store"][r]) & 0x7FFF for r in (100, 250, 254, 310, 500)] == [0, 1, 2, 3, 4])
    # ---- 3. a fence row beside a sink row; the first sink in row 0
    add("fence-beside-sink", [gc.mem(range(400)), gc.mem([10, 203]), gc.mem([10], G)],
        lambda g, c: _z(c)[10] & gr.REC_FENCE and not _z(c)[10] & gr.REC_SINK and _z(c)[11] & gr.REC_SINK and
        not _z(c)[11] & gr.REC_FENCE and gc.spilled(c, 8, 10))
    add("first-sink-row-0", [gc.mem([0], G), gc.mem(range(50))],
        lambda g, c: c.words(4)["first_sink"] == 0 and g["sink"][0] == 1 and g["n"] == 51)
    # ---- 4. 0, 1, 4, 5 and 11 predecessors, kept in slots, in spill rows (every slot busy; beyond kFarLds) and in registers
    fan = [gc.mem(range(311))] + [gc.mem([s, 300]) for s in (3, 40, 120, 200, 250, 260, 270, 280, 290, 295)] + \
          [gc.mem([s, 150]) for s in (100, 120, 140)] + [gc.mem([s, 160]) for s in (101, 121, 141, 151)]
    add("fan-in-0-1-4-5-11", fan,
        lambda g, c: {0, 1, 4, 5, 11} <= set(_npred(g)) and _npred(g)[300] == 11 and _npred(g)[150] == 4 and _npred(g)[160] == 5 and
        gc.spilled(c, 4, 3) and gc.spilled(c, 4, 40) and any(not gc.spilled(c, 8, r) for r in (250, 260, 270, 280, 290)) and
        (_z(c)[300] >> 24) == 1 and (_z(c)[160] >> 24) >= 1 and ((_z(c)[300] >> gr.REC_DIST_SHIFT) & 63) == 63 and
        ((_z(c)[150] >> gr.REC_DIST_SHIFT) & 63) == 50)
    # ---- 5. where the codes are kept: at the thresholds for a family of 3, and forty members with columns of their own
    two3, one3 = rows_that_fit(3, 2), rows_that_fit(3, 1)
    add("f3-two-last", ladder(two3), lambda g, c: g["n"] == two3 and fit(two3, 3) == "two" and fit(two3 + 1, 3) == "one", big=True)
    add("f3-one-first", ladder(two3 + 1), lambda g, c: g["n"] == two3 + 1 and fit(g["n"], 3) == "one", big=True)
    add("f3-one-last", ladder(one3), lambda g, c: g["n"] == one3 and fit(one3, 3) == "one" and fit(one3 + 1, 3) == "global", big=True)
    add("f3-global-first", ladder(one3 + 1), lambda g, c: g["n"] == one3 + 1 and fit(g["n"], 3) == "global", big=True)
    add("f40-two", disjoint(40, 80), lambda g, c: g["n"] == 3200 and fit(3200, 40) == "two" and int(g["sink"].sum()) == 40, big=True)
    add("f40-one", disjoint(40, 125), lambda g, c: g["n"] == 5000 and fit(5000, 40) == "one", big=True)
    add("f40-global", disjoint(40, 250), lambda g, c: g["n"] == 10000 and fit(10000, 40) == "global" and g["n"] < gc.FIRST_NCAP, big=True)
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# launches of families of one size (the launch's largest family sets the room), each with every place the codes are kept
GROUPS = {
    "f3": ["rows-17", "rows-513", "f3-two-last", "f3-one-first", "f3-one-last", "f3-global-first"],
    "f40": ["f40-two", "f40-one", "f40-global"],
}


def rings_of(case):
    return RINGS if case.big else RINGS_MORE


def bound_of(g, kappa64):
    """Step 9 restated: per node (R = the sum of the column maxima right of the node's column, C = the occupied columns
    right of it), and the smallest column maximum.  Units: common.h prune_gain_units."""
    from tests import gate_cases
    n = g["n"]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0xFFFFFFFF
    units = np.array([gate_cases.gain_units(w, kappa64) for w in g["weight"]], np.int64)
    cols, col_of = np.unique(g["pos"], return_inverse=True)
    mx = np.zeros(len(cols), np.int64)
    np.maximum.at(mx, col_of, units)
    through = np.cumsum(mx)
    return (through[-1] - through)[col_of], (len(cols) - 1 - col_of).astype(np.int64), int(mx.min())


def query_of(case, length):
    """The first `length` bases of the first member, every seventh substituted."""
    m = case.family()[0]
    q = ((m >> 24) & 0x0F).astype(np.uint8)[:length].copy()
    for i in range(2, len(q), 7):
        q[i] = {A: G, G: C, C: U}.get(int(q[i]), A)
    return q
