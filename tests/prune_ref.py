"""The check of the DP kernel's certified row skip against the oracle's planes (mesh_dp.hip PRUNE), shared
by tests/test_gpu_prune.py and tests/test_gpu_gates.py: every cell whose reference value is at or below the bound the
kernel ended up using is the reference's bit for bit -- value, value_midx, value_sidx --, every other cell is above its
bound."""
import numpy as np

from tests import util


def _bound_plane(info, rg_cols, N, L):
    """T(m, s) = U + min(a * r, R(m) - gmin * max(0, C(m) - r)), r = L-1-s, in units of 1/64, as float64 (common.h,
    "the bound")."""
    rg, cols = rg_cols
    a, gmin = float(info["prune_step"]), float(info["prune_gmin"])
    r = (L - 1 - np.arange(L, dtype=np.float64))[None, :]
    second = rg.astype(np.float64)[:, None] - gmin * np.maximum(0.0, cols.astype(np.float64)[:, None] - r)
    return info["ubound"] + np.minimum(a * r, second) / 64.0


def _check_planes(ctx, cells, vm, vs, val):
    N, L = val.shape
    info = ctx.dp_info(0)
    assert info["attempts"] >= 1, "the launch did not go through the skipping kernel"
    if np.isinf(info["ubound"]):     # third attempt: swept in full
        alive = np.ones((N, L), bool)
    else:
        T = _bound_plane(info, ctx.rgain(N), N, L)
        alive = cells["value"].astype(np.float64) <= T
        assert (val[~alive].astype(np.float64) > T[~alive]).all(), "a cell the reference has above its bound came out at or below it"
    assert (util.f32_bits(val)[alive] == util.f32_bits(cells["value"])[alive]).all()
    assert (vm[alive] == cells["value_midx"][alive]).all()
    assert (vs[alive] == cells["value_sidx"][alive]).all()
    return info, alive
