"""Generates tests/golden/gate_vectors.npz: for every case of tests/gate_cases.py the shape and one hash per plane
(util.MESH_PLANES) of the cell planes the REAL reference parts compute (oracle/_ref: the reference's dag<T>, its scoring
schemes, its cell loop -- ref_mesh_compute).  Run in the build container only:

    make -C oracle && python tests/golden/make_gate_vectors.py

Only case ids, shapes and hashes go in; the tests regenerate the inputs from the same seeds and compare the oracle
(tests/test_gates_cpu.py) -- and through it the GPU (tests/test_gpu_gates.py) -- with them.  Deterministic: a second run
writes the same bytes.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from tests import gate_cases as gc, util  # noqa: E402

R = po.ref()
R.ref_mesh_compute.argtypes = [C.c_void_p, po.u32p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float,
                               po.f32p, C.c_uint32, C.c_int, C.c_void_p]

ids, shapes, hashes, finite = [], [], [], []
dags = {}
for case in gc.all_cases():
    refs, fam_ids, qm = gc.family(case["fam"])
    key = (case["fam"], case["fs_weight"])
    if key not in dags:
        arrs = [np.ascontiguousarray(refs.seq(int(i))) for i in fam_ids]
        ptrs = (po.u32p * len(arrs))(*[a.ctypes.data_as(po.u32p) for a in arrs])
        ns = np.array([len(a) for a in arrs], np.uint32)
        dags[key] = R.ref_dag_build(ptrs, ns.ctypes.data_as(po.u32p), len(arrs), refs.width, case["fs_weight"])
    rd = dags[key]
    N = R.ref_dag_size(rd)
    qa = np.arange(len(qm), dtype=np.uint32) | (qm.astype(np.uint32) << 24)
    w = gc.case_weights(case)
    cells = np.zeros((N, len(qa)), po.CELL_DTYPE)
    R.ref_mesh_compute(rd, qa.ctypes.data_as(po.u32p), len(qa), -case["match"], -case["mismatch"], case["gap"], case["gapext"],
                       w.ctypes.data_as(po.f32p) if w is not None else None, len(w) if w is not None else 0,
                       int(case["forbid"]), cells.ctypes.data_as(C.c_void_p))
    ids.append(case["id"])
    shapes.append((N, len(qa)))
    hashes.append([util.plane_hash(cells[f]) for f in util.MESH_PLANES])
    finite.append(all(np.isfinite(cells[f]).all() for f in ("value", "gapm_val", "gaps_val")))
for rd in dags.values():
    R.ref_dag_free(rd)

assert all(finite), [i for i, ok in zip(ids, finite) if not ok]
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gate_vectors.npz")
out = dict(case_id=np.array(ids), shape=np.array(shapes, np.int64), hash=np.array(hashes, np.uint64))
# (an .npz is a zip of .npy members; np.savez stamps each with the time of day -- written here with a fixed one, so
# that a second run gives the same bytes)
import io  # noqa: E402
import zipfile  # noqa: E402
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
    for name, arr in out.items():
        buf = io.BytesIO()
        np.lib.format.write_array(buf, arr, allow_pickle=False)
        zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
print("wrote", path, os.path.getsize(path), "bytes;", len(ids), "cases")
