"""ctypes view of the C ABI in include/sina_hip.h (sina_amd/libsina_hip.so).

This is what a foreign host (SINA's C++ stages, or any other FFI) binds; the
Python layer adds nothing but argument marshalling.  The library is loaded from
the package directory (in-tree build) and loading fails loudly if it is missing:
there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SINA_HIP_LIB: the profiling build of the same library, tools only)
LIB_PATH = os.path.abspath(os.environ["SINA_HIP_LIB"]) if os.environ.get("SINA_HIP_LIB") else os.path.join(_HERE, "libsina_hip.so")

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)
i16p = C.POINTER(C.c_int16)
u16p = C.POINTER(C.c_uint16)

# every extern "C" symbol include/sina_hip.h declares
ABI_SYMBOLS = [
    "sina_hip_abi_version", "sina_hip_last_error", "sina_hip_init", "sina_hip_fork", "sina_hip_prewarm", "sina_hip_destroy",
    "sina_hip_sync",
    "sina_hip_upload_refs", "sina_hip_build_index", "sina_hip_download_index", "sina_hip_upload_index", "sina_hip_store_view_get",
    "sina_hip_store_alloc_like", "sina_hip_kmer_topk", "sina_hip_kmer_scores", "sina_hip_compare",
    "sina_hip_align_params_default", "sina_hip_staged_out_pos", "sina_hip_align_graphs", "sina_hip_align_families",
    "sina_hip_align_profiles", "sina_hip_debug_family_profile", "sina_hip_debug_family_profile_words",
    "sina_hip_debug_mesh", "sina_hip_debug_family_graph", "sina_hip_debug_family_graph_words", "sina_hip_debug_dp_info", "sina_hip_debug_rgain", "sina_hip_debug_chain_rows", "sina_hip_get_stats",
    "sina_hip_align_graphs_any", "sina_hip_debug_mesh_wide", "sina_hip_wide_queries", "sina_hip_last_error_is_limit",
    "sina_hip_kmer_topk_any", "sina_hip_kmer_scores_any", "sina_hip_long_queries", "sina_hip_big_select_queries",
    "sina_hip_align_graphs_wsets", "sina_hip_align_families_wsets",
    "sina_hip_match_count", "sina_hip_kmer_topk_match", "sina_hip_match_stats",
    "sina_hip_family_row_words", "sina_hip_family_cascade", "sina_hip_kmer_topk_family", "sina_hip_family_stats",
    "sina_hip_upload_name_order", "sina_hip_compare_rank", "sina_hip_kmer_topk_rank", "sina_hip_rank_stats",
    "sina_hip_upload_pairs", "sina_hip_pair_counts", "sina_hip_pair_stats",
    "sina_hip_align_count_pairs", "sina_hip_staged_pair_counts", "sina_hip_pair_inplace_stats",
    "sina_hip_align_count_identity", "sina_hip_staged_identity", "sina_hip_identity_inplace_stats",
    "sina_hip_align_rank", "sina_hip_staged_rank", "sina_hip_rank_inplace_stats",
    "sina_hip_show_dist", "sina_hip_show_dist_stats",
    "sina_hip_find_bases", "sina_hip_find_bases_stats",
    "sina_hip_kmer_topk_turn", "sina_hip_turn_stats",
    "sina_hip_staged_shift_log", "sina_hip_assemble_stats", "sina_hip_debug_assemble", "sina_hip_debug_assemble_ms",
]

# include/sina_hip.h: SINA_ASSEMBLE_SHIFT, SINA_HIP_SHIFT_LOG
ASSEMBLE_SHIFT = 2
SHIFT_LOG = 32

# include/sina_hip.h, sina_hip_staged_rank: words of a query's row
RANK_ROW_WORDS = 130

# csrc/family_plan.h: the most entries a rule's family may have on the device
FAMILY_MAX_K = 1024


class FamilyRule(C.Structure):
    """sina_hip_family_rule: famfinder's options the cascade reads; the defaults are famfinder's."""
    _fields_ = [("fs_min", C.c_uint32), ("fs_max", C.c_uint32), ("fs_req_full", C.c_uint32), ("fs_full_len", C.c_uint32),
                ("fs_min_len", C.c_uint32), ("fs_cover_gene", C.c_uint32), ("fs_msc", C.c_float), ("fs_msc_max", C.c_float)]

    def __init__(self, fs_min=40, fs_max=40, fs_req_full=1, fs_full_len=1400, fs_min_len=150, fs_cover_gene=0, fs_msc=0.7,
                 fs_msc_max=2.0):
        super().__init__(fs_min, fs_max, fs_req_full, fs_full_len, fs_min_len, fs_cover_gene, fs_msc, fs_msc_max)

    @property
    def K(self):
        return max(self.fs_min, self.fs_max) + self.fs_req_full + 2 * self.fs_cover_gene

    @property
    def row_words(self):
        """2 + 2 K (the mirror of sina_hip_family_row_words, which also refuses K > FAMILY_MAX_K)."""
        return 2 + 2 * self.K


# include/sina_hip.h: SINA_CMP_COVER_*, in CMP_COVER_TYPE's order
COVER_RULES = ("abs", "query", "target", "overlap", "all", "average", "min", "max", "nogap")
RANK_MAX_RESULT = 64

# include/sina_hip.h: the fast k-mer / DP paths' query limit, the _any k-mer entries' limit, and the number of k-mer
# windows (by the index of their last base) the long count kernel takes per chunk
MAX_QUERY_LEN = 10240
MAX_LONG_QUERY_LEN = 32767
KMER_LONG_CHUNK = 10240


class AlignParams(C.Structure):
    _fields_ = [("match_score", C.c_float), ("mismatch_score", C.c_float), ("gap_penalty", C.c_float),
                ("gap_ext_penalty", C.c_float), ("fs_weight", C.c_float), ("overhang", C.c_int32),
                ("lowercase", C.c_int32), ("insertion", C.c_int32), ("weights", f32p),
                ("n_weights", C.c_uint32), ("assemble", C.c_int32)]


class GraphBatch(C.Structure):
    _fields_ = [("nq", C.c_uint32), ("node_off", u64p), ("edge_off", u64p), ("node_pos", u32p),
                ("node_mask", u8p), ("node_weight", f32p), ("pred_off", u32p), ("pred", u32p),
                ("succ_minpos", u32p), ("width", C.c_uint32), ("node_score16", f32p), ("self_score16", f32p)]


class AlignOut(C.Structure):
    _fields_ = [("end_m", C.c_uint32), ("end_s", C.c_uint32), ("raw", C.c_float), ("sum_weight", C.c_float),
                ("aligned_bases", C.c_int32), ("cutoff_head", C.c_int32), ("cutoff_tail", C.c_int32),
                ("n_out", C.c_uint32), ("status", C.c_int32), ("assembled", C.c_uint32),
                ("nast_total", C.c_uint32), ("nast_longest", C.c_uint32), ("nast_last_run", C.c_uint32)]


ALIGN_OUT_DTYPE = np.dtype([("end_m", "<u4"), ("end_s", "<u4"), ("raw", "<f4"), ("sum_weight", "<f4"),
                            ("aligned_bases", "<i4"), ("cutoff_head", "<i4"), ("cutoff_tail", "<i4"),
                            ("n_out", "<u4"), ("status", "<i4"), ("assembled", "<u4"), ("nast_total", "<u4"),
                            ("nast_longest", "<u4"), ("nast_last_run", "<u4")])


class StoreView(C.Structure):
    _fields_ = [("ref_ab", C.c_void_p), ("ref_ab_bytes", C.c_uint64), ("ref_off", C.c_void_p),
                ("ref_off_bytes", C.c_uint64), ("idx_offsets", C.c_void_p), ("idx_offsets_bytes", C.c_uint64),
                ("idx_ids", C.c_void_p), ("idx_ids_bytes", C.c_uint64), ("n_refs", C.c_uint32),
                ("width", C.c_uint32), ("k", C.c_uint32), ("nofast", C.c_uint32), ("n_postings", C.c_uint64),
                ("total_bases", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("dp_ms", C.c_double), ("backtrack_ms", C.c_double), ("graph_ms", C.c_double),
                ("kmer_count_ms", C.c_double), ("kmer_select_ms", C.c_double), ("dp_cells", C.c_uint64),
                ("postings", C.c_uint64), ("dp_launches", C.c_uint32), ("kmer_launches", C.c_uint32),
                ("compare_ms", C.c_double), ("compare_bases", C.c_uint64), ("compare_launches", C.c_uint32),
                ("n_dense_lists", C.c_uint32), ("dp_busy_ms", C.c_double), ("dags_built", C.c_uint64),
                ("dags_used", C.c_uint64), ("dp_rows", C.c_uint64), ("dp_rows_swept", C.c_uint64),
                ("dp_cells_swept", C.c_uint64), ("dp_queries_pruned", C.c_uint64), ("dp_second_attempts", C.c_uint64),
                ("dp_full_sweeps", C.c_uint64), ("dp_prune_rho", C.c_double), ("graph_bytes", C.c_uint64),
                ("graph_launches", C.c_uint32), ("kmer_queries", C.c_uint32), ("scout_ms", C.c_double),
                ("scout_launches", C.c_uint32), ("pad_", C.c_uint32)]


class DpInfo(C.Structure):
    _fields_ = [("end_m", C.c_uint32), ("end_s", C.c_uint32), ("raw", C.c_float), ("status", C.c_int32),
                ("rows_swept", C.c_uint32), ("cells_swept", C.c_uint32), ("attempts", C.c_uint32),
                ("gain0", C.c_float), ("ubound", C.c_float), ("prune_step", C.c_uint32), ("prune_gmin", C.c_uint32),
                ("scout", C.c_float), ("kernel", C.c_uint32)]


# include/sina_hip.h: SINA_DP_KERNEL_*, what DpInfo.kernel holds
DP_KERNELS = ("none", "simple", "simple_skip", "generic_below", "generic", "weighted", "forbid", "weighted_forbid")


_lib = None


def load():
    """Loads libsina_hip.so; raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("sina_amd/libsina_hip.so is missing: run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.sina_hip_abi_version.restype = C.c_int
    L.sina_hip_last_error.restype = C.c_char_p
    L.sina_hip_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.sina_hip_fork.argtypes = [vp, C.POINTER(vp)]
    L.sina_hip_prewarm.argtypes = [vp, C.c_int]
    L.sina_hip_destroy.argtypes = [vp]
    L.sina_hip_destroy.restype = None
    L.sina_hip_sync.argtypes = [vp]
    L.sina_hip_staged_out_pos.restype = C.POINTER(C.c_uint32)
    L.sina_hip_staged_out_pos.argtypes = [vp]
    L.sina_hip_upload_refs.argtypes = [vp, u32p, u64p, C.c_uint32, C.c_uint32]
    L.sina_hip_build_index.argtypes = [vp, C.c_uint, C.c_int]
    L.sina_hip_upload_index.argtypes = [vp, C.c_uint, C.c_int, u32p, u32p, C.c_uint64]
    L.sina_hip_download_index.argtypes = [vp, u32p, u32p]
    L.sina_hip_store_view_get.argtypes = [vp, C.POINTER(StoreView)]
    L.sina_hip_store_alloc_like.argtypes = [vp, C.POINTER(StoreView)]
    L.sina_hip_kmer_topk.argtypes = [vp, u8p, u64p, C.c_uint32, C.c_uint32, u32p, f32p, u32p]
    L.sina_hip_kmer_scores.argtypes = [vp, u8p, C.c_uint32, i16p]
    L.sina_hip_compare.argtypes = [vp, u32p, u64p, C.c_uint32, u32p, u64p, C.c_int, C.c_int, C.c_void_p]
    L.sina_hip_align_params_default.argtypes = [C.POINTER(AlignParams)]
    L.sina_hip_align_params_default.restype = None
    L.sina_hip_align_graphs.argtypes = [vp, C.POINTER(GraphBatch), u8p, u64p, C.POINTER(AlignParams),
                                        C.POINTER(AlignOut), u32p]
    L.sina_hip_align_graphs_any.argtypes = L.sina_hip_align_graphs.argtypes
    L.sina_hip_wide_queries.argtypes = [vp, u64p]
    L.sina_hip_kmer_topk_any.argtypes = L.sina_hip_kmer_topk.argtypes
    L.sina_hip_kmer_scores_any.argtypes = L.sina_hip_kmer_scores.argtypes
    L.sina_hip_long_queries.argtypes = [vp, u64p]
    L.sina_hip_big_select_queries.argtypes = [vp, u64p]
    L.sina_hip_match_count.argtypes = [vp, u32p, u64p, C.c_uint32, u32p, u64p, u16p]
    L.sina_hip_kmer_topk_match.argtypes = [vp, u32p, u64p, C.c_uint32, C.c_uint32, u32p, f32p, u32p, u16p]
    L.sina_hip_match_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    rulep = C.POINTER(FamilyRule)
    L.sina_hip_family_row_words.argtypes = [rulep, u32p]
    L.sina_hip_family_cascade.argtypes = [vp, u32p, f32p, u16p, u64p, u32p, C.c_uint32, rulep, u32p, u64p, u32p]
    L.sina_hip_kmer_topk_family.argtypes = [vp, u32p, u64p, C.c_uint32, C.c_uint32, rulep, u32p, u64p, u32p]
    L.sina_hip_family_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p, u64p]
    L.sina_hip_upload_name_order.argtypes = [vp, u32p, C.c_uint32]
    L.sina_hip_compare_rank.argtypes = [vp, u32p, u64p, C.c_uint32, u32p, u64p, C.c_int, C.c_int, C.c_int, C.c_uint32, u32p, f32p,
                                        u32p, u32p]
    L.sina_hip_kmer_topk_rank.argtypes = [vp, u32p, u64p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, u32p,
                                          f32p, u32p, u32p]
    L.sina_hip_rank_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_upload_pairs.argtypes = [vp, u32p, C.c_uint32]
    L.sina_hip_pair_counts.argtypes = [vp, u32p, u64p, C.c_uint32, u32p]
    L.sina_hip_pair_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_align_count_pairs.argtypes = [vp, C.c_int]
    L.sina_hip_staged_pair_counts.restype = C.POINTER(C.c_uint32)
    L.sina_hip_staged_pair_counts.argtypes = [vp]
    L.sina_hip_pair_inplace_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p]
    L.sina_hip_align_count_identity.argtypes = [vp, C.c_int]
    L.sina_hip_staged_identity.restype = C.POINTER(C.c_uint32)
    L.sina_hip_staged_identity.argtypes = [vp]
    L.sina_hip_identity_inplace_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_show_dist.argtypes = [vp, u32p, u64p, u32p, u64p, C.c_uint32, u32p, u64p, u32p]
    L.sina_hip_show_dist_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_find_bases.argtypes = [vp, u8p, u64p, C.c_uint32, u32p, u64p, u32p]
    L.sina_hip_find_bases_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_kmer_topk_turn.argtypes = [vp, u8p, u64p, C.c_uint32, C.c_uint32, C.c_int, u8p, f32p, u32p, f32p, u32p]
    L.sina_hip_turn_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_align_rank.argtypes = [vp, C.c_int, C.c_uint, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32]
    L.sina_hip_staged_rank.restype = C.POINTER(C.c_uint32)
    L.sina_hip_staged_rank.argtypes = [vp]
    L.sina_hip_rank_inplace_stats.argtypes = [vp, C.POINTER(C.c_double), u64p, u64p, u64p]
    L.sina_hip_staged_shift_log.restype = C.POINTER(C.c_uint32)
    L.sina_hip_staged_shift_log.argtypes = [vp]
    L.sina_hip_assemble_stats.argtypes = [vp, u64p, u64p, u64p, u64p]
    L.sina_hip_debug_assemble.argtypes = [vp, C.POINTER(AlignParams), C.c_uint32, u8p, u64p, C.c_uint32, C.POINTER(AlignOut), u32p]
    L.sina_hip_debug_assemble_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.sina_hip_last_error_is_limit.restype = C.c_int
    L.sina_hip_debug_mesh_wide.argtypes = [vp, C.POINTER(GraphBatch), u8p, C.c_uint32, C.POINTER(AlignParams),
                                           u32p, u32p, f32p]
    L.sina_hip_align_families.argtypes = [vp, u32p, u64p, C.c_uint32, u8p, u64p, C.POINTER(AlignParams),
                                          C.POINTER(AlignOut), u32p]
    L.sina_hip_align_profiles.argtypes = L.sina_hip_align_families.argtypes
    L.sina_hip_align_graphs_wsets.argtypes = [vp, C.POINTER(GraphBatch), u8p, u64p, C.POINTER(AlignParams), u32p, C.c_uint32,
                                              C.POINTER(AlignOut), u32p]
    L.sina_hip_align_families_wsets.argtypes = [vp, u32p, u64p, C.c_uint32, u8p, u64p, C.POINTER(AlignParams), u32p,
                                                C.c_uint32, C.POINTER(AlignOut), u32p]
    L.sina_hip_debug_family_profile.argtypes = [vp, u32p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, u32p, u32p,
                                                f32p, f32p, C.c_uint32]
    L.sina_hip_debug_family_profile_words.argtypes = [vp, u32p, C.c_uint32, u32p, u32p, u32p, u32p, u32p, C.c_uint32]
    L.sina_hip_debug_mesh.argtypes = [vp, C.POINTER(GraphBatch), u8p, C.c_uint32, C.POINTER(AlignParams),
                                      u32p, u32p, f32p, C.c_int]
    L.sina_hip_debug_family_graph.argtypes = [vp, u32p, C.c_uint32, C.c_float, C.c_uint32, u32p, u32p, u32p, u8p,
                                              f32p, u32p, u32p, u32p, u8p, u32p, C.c_uint32, C.c_uint32]
    L.sina_hip_debug_family_graph_words.argtypes = [vp, u32p, C.c_uint32, C.c_float, C.c_uint32, u32p, u32p, u32p, u32p,
                                                    u32p, u32p, C.c_uint32, C.c_uint32]
    L.sina_hip_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.sina_hip_debug_dp_info.argtypes = [vp, C.c_uint32, C.POINTER(DpInfo)]
    L.sina_hip_debug_rgain.argtypes = [vp, C.c_uint32, u32p, u32p]
    _lib = L
    return L


class SinaHipError(RuntimeError):
    pass


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def read_counters(fn, args, fields, check):
    """Reads a C getter of counters: fn(*args, out...) with one out-parameter per (key, ctype) of `fields`, in their order;
    its return code goes to `check`.  Returns dict(key=value) in that order, float for c_double and int otherwise."""
    outs = [t() for _, t in fields]
    check(fn(*args, *[C.byref(o) for o in outs]))
    return {k: float(o.value) if t is C.c_double else int(o.value) for (k, t), o in zip(fields, outs)}


KERNEL_MS = [("kernel_ms", C.c_double)]


def u64_fields(*keys):
    return [(k, C.c_uint64) for k in keys]


class Context:
    """Owns one sina_hip_ctx (one GPU, one stream)."""

    def __init__(self, device=0, _parent=None):
        self.L = load()
        self.h = C.c_void_p()
        if _parent is None:
            self._check(self.L.sina_hip_init(device, C.byref(self.h)))
        else:
            self._check(self.L.sina_hip_fork(_parent.h, C.byref(self.h)))
        self._parent = _parent  # keeps the owner of the store alive
        self.device = device
        self.n_refs = 0 if _parent is None else _parent.n_refs

    def fork(self):
        """A context with its own stream and scratch that shares this one's store and index."""
        return Context(self.device, _parent=self)

    def _check(self, rc):
        if rc != 0:
            raise SinaHipError(self.L.sina_hip_last_error().decode())

    def _counters(self, fn, fields):
        return read_counters(fn, (self.h,), fields, self._check)

    def close(self):
        if self.h:
            self.L.sina_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- store
    def upload_refs(self, ab, off, width):
        ab = _c(ab, np.uint32)
        off = _c(off, np.uint64)
        self._keep = (ab, off)
        self.n_refs = len(off) - 1
        self._check(self.L.sina_hip_upload_refs(self.h, _ptr(ab, u32p), _ptr(off, u64p), self.n_refs, width))

    def build_index(self, k=10, nofast=False):
        self._check(self.L.sina_hip_build_index(self.h, k, int(nofast)))

    def upload_index(self, k, nofast, offsets, ids):
        offsets = _c(offsets, np.uint32)
        ids = _c(ids, np.uint32)
        self._check(self.L.sina_hip_upload_index(self.h, k, int(nofast), _ptr(offsets, u32p), _ptr(ids, u32p),
                                                 len(ids)))

    def download_index(self):
        """The device index as CSR: (offsets u32[4^k+1], ids u32[n_postings])."""
        v = self.store_view()
        off = np.zeros((1 << (2 * v.k)) + 1, np.uint32)
        ids = np.zeros(max(int(v.n_postings), 1), np.uint32)
        self._check(self.L.sina_hip_download_index(self.h, _ptr(off, u32p), _ptr(ids, u32p)))
        return off, ids[:int(v.n_postings)]

    def store_view(self):
        v = StoreView()
        self._check(self.L.sina_hip_store_view_get(self.h, C.byref(v)))
        return v

    def store_alloc_like(self, view):
        self._check(self.L.sina_hip_store_alloc_like(self.h, C.byref(view)))
        self.n_refs = view.n_refs
        return view

    # ---- k-mer search
    def kmer_topk(self, qmask, qoff, mx, long_ok=False):
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        nq = len(qoff) - 1
        mx_eff = max(1, min(mx, self.n_refs))
        ids = np.zeros((nq, mx_eff), np.uint32)
        sc = np.zeros((nq, mx_eff), np.float32)
        n = np.zeros(nq, np.uint32)
        fn = self.L.sina_hip_kmer_topk_any if long_ok else self.L.sina_hip_kmer_topk
        self._check(fn(self.h, _ptr(qmask, u8p), _ptr(qoff, u64p), nq, mx, _ptr(ids, u32p), _ptr(sc, f32p), _ptr(n, u32p)))
        return ids, sc, n

    def kmer_scores(self, qmask, long_ok=False):
        qmask = _c(qmask, np.uint8)
        s = np.zeros(self.n_refs, np.int16)
        fn = self.L.sina_hip_kmer_scores_any if long_ok else self.L.sina_hip_kmer_scores
        self._check(fn(self.h, _ptr(qmask, u8p), len(qmask), _ptr(s, i16p)))
        return s

    def kmer_topk_any(self, qmask, qoff, mx):
        """kmer_topk for queries of up to MAX_LONG_QUERY_LEN bases (the longer ones on the long count kernel)."""
        return self.kmer_topk(qmask, qoff, mx, long_ok=True)

    def kmer_scores_any(self, qmask):
        return self.kmer_scores(qmask, long_ok=True)

    def kmer_topk_turn(self, qmask, qoff, mx, all):
        """kmer_topk_any for the orientation of every query that scores best (famfinder's --turn): the device makes the
        tried orientations -- o = 0 and 3, with `all` 0, 3, 1, 2; o = (bit 0: reversed) | (bit 1: complemented) --
        searches them and chooses the first strictly largest top-1 score above 0 over o = 0 .. 3, else 0.  Returns
        (turn uint8 [nq], top1 float32 [nq, 4] by orientation, ids, scores, n): the last three as kmer_topk_any's for the
        chosen orientation's mask bytes."""
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        nq = len(qoff) - 1
        mx_eff = max(1, min(mx, self.n_refs))
        turn = np.zeros(nq, np.uint8)
        top1 = np.zeros((nq, 4), np.float32)
        ids = np.zeros((nq, mx_eff), np.uint32)
        sc = np.zeros((nq, mx_eff), np.float32)
        n = np.zeros(nq, np.uint32)
        self._check(self.L.sina_hip_kmer_topk_turn(self.h, _ptr(qmask, u8p), _ptr(qoff, u64p), nq, mx, 1 if all else 0, _ptr(turn, u8p),
                                                   _ptr(top1, f32p), _ptr(ids, u32p), _ptr(sc, f32p), _ptr(n, u32p)))
        return turn, top1, ids, sc, n

    def turn_stats(self):
        """The orient and pick kernels on this context so far: dict(kernel_ms, queries, turned, launches)."""
        return self._counters(self.L.sina_hip_turn_stats, KERNEL_MS + u64_fields("queries", "turned", "launches"))

    def long_queries(self):
        """Queries the long k-mer count kernel has counted on this context so far."""
        return self._counters(self.L.sina_hip_long_queries, u64_fields("n"))["n"]

    def big_select_queries(self):
        """Queries the big select (more than 4096 candidates per query) has ranked on this context so far."""
        return self._counters(self.L.sina_hip_big_select_queries, u64_fields("n"))["n"]

    # ---- alignment
    @staticmethod
    def params(weights=None, **kw):
        p = AlignParams()
        load().sina_hip_align_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        if weights is not None:
            w = _c(weights, np.float32)
            p._keep = w
            p.weights = _ptr(w, f32p)
            p.n_weights = len(w)
        return p

    @staticmethod
    def graph_batch(graphs, width, node_score16=None, self_score16=None):
        """graphs: list of dicts with pos, mask, weight, pred_off, pred[, succ_minpos].
        node_score16 / self_score16: a profile batch (--fs-no-graph, sina_hip_graph_batch): float32
        [total nodes, 16] match terms per node and query iupac mask, and the 16 self-comparison terms."""
        nq = len(graphs)
        node_off = np.zeros(nq + 1, np.uint64)
        edge_off = np.zeros(nq + 1, np.uint64)
        for i, g in enumerate(graphs):
            node_off[i + 1] = node_off[i] + len(g["pos"])
            edge_off[i + 1] = edge_off[i] + len(g["pred"])
        cat = lambda key, dt: _c(np.concatenate([np.asarray(g[key]) for g in graphs]) if nq else [], dt)
        arrs = dict(node_off=node_off, edge_off=edge_off, node_pos=cat("pos", np.uint32),
                    node_mask=cat("mask", np.uint8), node_weight=cat("weight", np.float32),
                    pred_off=cat("pred_off", np.uint32), pred=cat("pred", np.uint32))
        if nq and all("succ_minpos" in g for g in graphs):
            arrs["succ_minpos"] = cat("succ_minpos", np.uint32)
        gb = GraphBatch()
        gb.nq = nq
        gb.node_off = _ptr(arrs["node_off"], u64p)
        gb.edge_off = _ptr(arrs["edge_off"], u64p)
        gb.node_pos = _ptr(arrs["node_pos"], u32p)
        gb.node_mask = _ptr(arrs["node_mask"], u8p)
        gb.node_weight = _ptr(arrs["node_weight"], f32p)
        gb.pred_off = _ptr(arrs["pred_off"], u32p)
        gb.pred = _ptr(arrs["pred"], u32p)
        gb.succ_minpos = _ptr(arrs["succ_minpos"], u32p) if "succ_minpos" in arrs else None
        gb.width = width
        if node_score16 is not None:
            arrs["node_score16"] = _c(np.asarray(node_score16).reshape(-1), np.float32)
            arrs["self_score16"] = _c(self_score16, np.float32)
            assert len(arrs["node_score16"]) == 16 * int(node_off[nq]) and len(arrs["self_score16"]) == 16
            gb.node_score16 = _ptr(arrs["node_score16"], f32p)
            gb.self_score16 = _ptr(arrs["self_score16"], f32p)
        gb._keep = arrs
        return gb

    def align_graphs(self, gb, qmask, qoff, params=None):
        params = params or self.params()
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        self._align_nq = len(qoff) - 1                  # (staged_pair_counts: rows of the last align call)
        out = np.zeros(gb.nq, ALIGN_OUT_DTYPE)
        pos = np.zeros(max(len(qmask), 1), np.uint32)
        self._check(self.L.sina_hip_align_graphs(self.h, C.byref(gb), _ptr(qmask, u8p), _ptr(qoff, u64p),
                                                 C.byref(params), out.ctypes.data_as(C.POINTER(AlignOut)),
                                                 _ptr(pos, u32p)))
        return out, pos

    def align_graphs_any(self, gb, qmask, qoff, params=None, staged=False):
        """align_graphs without the fast path's limits: a query the fast kernel cannot take goes through the wide
        kernel.  staged: pass out_pos == NULL and read the columns from the context's staging buffer."""
        params = params or self.params()
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        self._align_nq = len(qoff) - 1                  # (staged_pair_counts: rows of the last align call)
        out = np.zeros(gb.nq, ALIGN_OUT_DTYPE)
        pos = np.zeros(max(len(qmask), 1), np.uint32)
        self._check(self.L.sina_hip_align_graphs_any(self.h, C.byref(gb), _ptr(qmask, u8p), _ptr(qoff, u64p),
                                                     C.byref(params), out.ctypes.data_as(C.POINTER(AlignOut)),
                                                     None if staged else _ptr(pos, u32p)))
        if staged:
            n = int(qoff[-1] - qoff[0])
            pos[:n] = np.ctypeslib.as_array(self.L.sina_hip_staged_out_pos(self.h), shape=(max(n, 1),))[:n]
        return out, pos

    def wide_queries(self):
        """Queries the wide kernel has aligned on this context so far."""
        return self._counters(self.L.sina_hip_wide_queries, u64_fields("n"))["n"]

    def last_error_is_limit(self):
        """True if this thread's last failed call was refused for exceeding a documented limit of the fast path."""
        return bool(self.L.sina_hip_last_error_is_limit())

    def debug_mesh_wide(self, gb, qmask, params=None, want_value=True):
        """The wide kernel's planes of ONE query: (value_midx, value_sidx, value), each [N, L]."""
        params = params or self.params()
        qmask = _c(qmask, np.uint8)
        n = int(gb._keep["node_off"][1])
        L = len(qmask)
        vm = np.zeros((n, L), np.uint32)
        vs = np.zeros((n, L), np.uint32)
        val = np.zeros((n, L), np.float32) if want_value else None
        self._check(self.L.sina_hip_debug_mesh_wide(self.h, C.byref(gb), _ptr(qmask, u8p), L, C.byref(params),
                                                    _ptr(vm, u32p), _ptr(vs, u32p),
                                                    _ptr(val, f32p) if want_value else None))
        return vm, vs, val

    def compare(self, q_ab, q_off, cand_ids, cand_off, iupac=0, filter_lc=False):
        """Search-stage comparison: int32 [n candidates][6] = only_a_overhang, only_b_overhang, only_a,
        only_b, match, mismatch of every (query, candidate) pair."""
        q_ab = _c(q_ab, np.uint32)
        q_off = _c(q_off, np.uint64)
        cand_ids = _c(cand_ids, np.uint32)
        cand_off = _c(cand_off, np.uint64)
        out = np.zeros((max(len(cand_ids), 1), 6), np.int32)
        self._check(self.L.sina_hip_compare(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), len(q_off) - 1,
                                            _ptr(cand_ids, u32p), _ptr(cand_off, u64p), int(iupac),
                                            int(filter_lc), out.ctypes.data_as(C.c_void_p)))
        return out[:len(cand_ids)]

    def match_counts(self, q_ab, q_off, cand_ids, cand_off):
        """Famfinder's identity filter: uint16 [n candidates] = the `match` counter (optimistic IUPAC rule, no
        lower-case filter) of every (query, candidate) pair; identity = float32(match) / float32(len(query))."""
        q_ab = _c(q_ab, np.uint32)
        q_off = _c(q_off, np.uint64)
        cand_ids = _c(cand_ids, np.uint32)
        cand_off = _c(cand_off, np.uint64)
        out = np.zeros(max(len(cand_ids), 1), np.uint16)
        self._check(self.L.sina_hip_match_count(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), len(q_off) - 1,
                                                 _ptr(cand_ids, u32p), _ptr(cand_off, u64p), _ptr(out, u16p)))
        return out[:len(cand_ids)]

    def kmer_topk_match(self, q_ab, q_off, mx):
        """kmer_topk_any for queries given as packed aligned bases (column | mask << 24), plus the match count of
        every candidate returned: (ids, scores, n, match), match uint16 [nq, min(mx, n_refs)]."""
        q_ab = _c(q_ab, np.uint32)
        q_off = _c(q_off, np.uint64)
        nq = len(q_off) - 1
        mx_eff = max(1, min(mx, self.n_refs))
        ids = np.zeros((nq, mx_eff), np.uint32)
        sc = np.zeros((nq, mx_eff), np.float32)
        n = np.zeros(nq, np.uint32)
        mt = np.zeros((nq, mx_eff), np.uint16)
        self._check(self.L.sina_hip_kmer_topk_match(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), nq, mx, _ptr(ids, u32p),
                                                    _ptr(sc, f32p), _ptr(n, u32p), _ptr(mt, u16p)))
        return ids, sc, n, mt

    def match_stats(self):
        """The match-count kernel on this context so far: dict(kernel_ms, pairs, cand_bases, launches)."""
        return self._counters(self.L.sina_hip_match_stats, KERNEL_MS + u64_fields("pairs", "cand_bases", "launches"))

    def family_row_words(self, rule):
        """Words of a query's row under `rule` (FamilyRule): 2 + 2 K; a rule over the cap raises (a limit)."""
        w = C.c_uint32(0)
        self._check(self.L.sina_hip_family_row_words(C.byref(rule), C.byref(w)))
        return int(w.value)

    @staticmethod
    def _self_lists(self_ids, self_off):
        if self_ids is None:
            return None, None, None, None
        ids = _c(np.concatenate([np.asarray(self_ids, np.uint32), np.zeros(1, np.uint32)]), np.uint32)   # (never empty)
        off = _c(self_off, np.uint64)
        return ids, off, _ptr(ids, u32p), _ptr(off, u64p)

    def family_cascade(self, cand_ids, cand_scores, cand_match, cand_off, q_bases, rule, self_ids=None, self_off=None):
        """Famfinder's filter cascade over the caller's ranked lists: uint32 [nq, 2 + 2 K] rows (kept, flags, K ids,
        K score bit patterns).  cand_match: None where rule.fs_msc_max >= 1."""
        cand_off = _c(cand_off, np.uint64)
        nq = len(cand_off) - 1
        ids = _c(np.concatenate([np.asarray(cand_ids, np.uint32), np.zeros(1, np.uint32)]), np.uint32)
        sc = _c(np.concatenate([np.asarray(cand_scores, np.float32), np.zeros(1, np.float32)]), np.float32)
        mt = None if cand_match is None else _c(np.concatenate([np.asarray(cand_match, np.uint16), np.zeros(1, np.uint16)]), np.uint16)
        qb = _c(np.concatenate([np.asarray(q_bases, np.uint32), np.zeros(1, np.uint32)]), np.uint32)
        keep = self._self_lists(self_ids, self_off)
        rows = np.zeros((nq, rule.row_words), np.uint32)
        self._check(self.L.sina_hip_family_cascade(self.h, _ptr(ids, u32p), _ptr(sc, f32p), None if mt is None else _ptr(mt, u16p),
                                                   _ptr(cand_off, u64p), _ptr(qb, u32p), nq, C.byref(rule), keep[2], keep[3],
                                                   _ptr(rows, u32p) if rows.size else None))
        return rows

    def kmer_topk_family(self, q_ab, q_off, mx, rule, self_ids=None, self_off=None):
        """kmer_topk_match's search with the cascade behind it, on the device: uint32 [nq, 2 + 2 K] rows."""
        q_ab = _c(np.concatenate([np.asarray(q_ab, np.uint32), np.zeros(1, np.uint32)]), np.uint32)
        q_off = _c(q_off, np.uint64)
        nq = len(q_off) - 1
        keep = self._self_lists(self_ids, self_off)
        rows = np.zeros((nq, rule.row_words), np.uint32)
        self._check(self.L.sina_hip_kmer_topk_family(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), nq, mx, C.byref(rule),
                                                     keep[2], keep[3], _ptr(rows, u32p) if rows.size else None))
        return rows

    def family_stats(self):
        """The cascade kernel on this context so far: dict(kernel_ms, queries, candidates_listed, candidates_scanned,
        launches)."""
        return self._counters(self.L.sina_hip_family_stats,
                              KERNEL_MS + u64_fields("queries", "candidates_listed", "candidates_scanned", "launches"))

    def upload_name_order(self, rank):
        """rank[id] = position of reference id's name in ascending byte-wise order (a permutation of 0..n_refs-1)."""
        rank = _c(rank, np.uint32)
        self._check(self.L.sina_hip_upload_name_order(self.h, _ptr(rank, u32p), len(rank)))

    @staticmethod
    def _cover(cover):
        return COVER_RULES.index(cover) if isinstance(cover, str) else int(cover)

    def compare_rank(self, q_ab, q_off, cand_ids, cand_off, iupac=0, filter_lc=False, cover="query", max_result=10, out=None):
        """Search-stage comparison, scored and ranked on the device: (ids uint32 [nq, max_result], scores float32
        [nq, max_result], n uint32 [nq], flag uint32 [nq]).  cand_ids None: every reference for every query.
        out: the four arrays to write into (a test of "outputs untouched")."""
        q_ab = _c(q_ab, np.uint32)
        q_off = _c(q_off, np.uint64)
        nq = len(q_off) - 1
        rows = max(int(max_result), 1)
        ids, sc, n, flag = out if out is not None else (np.zeros((nq, rows), np.uint32), np.zeros((nq, rows), np.float32),
                                                        np.zeros(nq, np.uint32), np.zeros(nq, np.uint32))
        if cand_ids is None:
            cp, op = None, None
        else:
            cand_ids = _c(cand_ids, np.uint32)
            cand_off = _c(cand_off, np.uint64)
            cp, op = _ptr(cand_ids, u32p), _ptr(cand_off, u64p)
        self._check(self.L.sina_hip_compare_rank(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), nq, cp, op, int(iupac), int(filter_lc),
                                                 self._cover(cover), int(max_result), _ptr(ids, u32p), _ptr(sc, f32p),
                                                 _ptr(n, u32p), _ptr(flag, u32p)))
        return ids, sc, n, flag

    def kmer_topk_rank(self, q_ab, q_off, kmer_candidates, iupac=0, filter_lc=False, cover="query", max_result=10):
        """kmer_topk_any for queries given as packed aligned bases, its candidates ranked as compare_rank ranks them,
        from the select's id rows on the device: (ids, scores, n, flag) as compare_rank's."""
        q_ab = _c(q_ab, np.uint32)
        q_off = _c(q_off, np.uint64)
        nq = len(q_off) - 1
        rows = max(int(max_result), 1)
        ids = np.zeros((nq, rows), np.uint32)
        sc = np.zeros((nq, rows), np.float32)
        n = np.zeros(nq, np.uint32)
        flag = np.zeros(nq, np.uint32)
        self._check(self.L.sina_hip_kmer_topk_rank(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), nq, int(kmer_candidates), int(iupac),
                                                   int(filter_lc), self._cover(cover), int(max_result), _ptr(ids, u32p),
                                                   _ptr(sc, f32p), _ptr(n, u32p), _ptr(flag, u32p)))
        return ids, sc, n, flag

    def rank_stats(self):
        """The rank kernels on this context so far: dict(kernel_ms, pairs, cand_bases, launches)."""
        return self._counters(self.L.sina_hip_rank_stats, KERNEL_MS + u64_fields("pairs", "cand_bases", "launches"))

    def upload_pairs(self, pairs):
        """The helix map for pair_counts: pairs[i] = partner column of column i, 0 = unpaired.  Empty or all zero: no map."""
        pairs = _c(pairs, np.uint32)
        self._check(self.L.sina_hip_upload_pairs(self.h, _ptr(pairs, u32p), len(pairs)))

    def pair_counts(self, q_ab, q_off, out=None):
        """The counters behind align_bp_score_slv: uint32 [nq, 6] = num, AG, AU, CG, GG, GU of every finished aligned
        sequence (packed words column | mask << 24, columns ascending).  out: the array to write into."""
        q_ab = _c(q_ab, np.uint32)
        q_off = _c(q_off, np.uint64)
        nq = len(q_off) - 1
        counts = out if out is not None else np.zeros((nq, 6), np.uint32)
        self._check(self.L.sina_hip_pair_counts(self.h, _ptr(q_ab, u32p), _ptr(q_off, u64p), nq, _ptr(counts, u32p)))
        return counts

    def pair_stats(self):
        """The pair-count kernel on this context so far: dict(kernel_ms, sequences, entries_visited, launches)."""
        return self._counters(self.L.sina_hip_pair_stats, KERNEL_MS + u64_fields("sequences", "entries_visited", "launches"))

    def show_dist(self, orig_ab, orig_off, al_ab, al_off, ref_ids, ref_off, out=None):
        """The counters behind --show-dist: uint32 [nq, 20] -- words 0..5 the input alignment against the finished one
        (exact IUPAC), 6..11 the input alignment and 12..17 the finished one against the closest relative of the list
        (optimistic), each in sina_hip_match_counts' order; word 18 that relative's reference id (0xFFFFFFFF: none);
        word 19 flags (bit 0: a member had no score, bit 1: computed).  The store needs a name order
        (upload_name_order).  out: the array to write into."""
        orig_ab, al_ab, ref_ids = _c(orig_ab, np.uint32), _c(al_ab, np.uint32), _c(ref_ids, np.uint32)
        orig_off, al_off, ref_off = _c(orig_off, np.uint64), _c(al_off, np.uint64), _c(ref_off, np.uint64)
        nq = len(orig_off) - 1
        rows = out if out is not None else np.zeros((nq, 20), np.uint32)
        self._check(self.L.sina_hip_show_dist(self.h, _ptr(orig_ab, u32p), _ptr(orig_off, u64p), _ptr(al_ab, u32p), _ptr(al_off, u64p),
                                              nq, _ptr(ref_ids, u32p), _ptr(ref_off, u64p), _ptr(rows, u32p)))
        return rows

    def show_dist_stats(self):
        """The show-dist kernel on this context so far: dict(kernel_ms, sequences, pairs, launches)."""
        return self._counters(self.L.sina_hip_show_dist_stats, KERNEL_MS + u64_fields("sequences", "pairs", "launches"))

    def find_bases(self, qmask, q_off, cand_ids, cand_off, out=None):
        """Where each candidate reference holds its query's bases (std::string::find over `mask & 0xF`): uint32, one word
        per candidate at out[cand_off[q] + i] -- the lowest start or 0xFFFFFFFF.  qmask / q_off: the queries' mask bytes
        and offsets [nq + 1]; cand_ids / cand_off: the candidates' reference ids and offsets [nq + 1] (sub-ranges of
        larger arrays included).  out: the array to write into, at least cand_off[-1] words."""
        qmask, cand_ids = _c(qmask, np.uint8), _c(cand_ids, np.uint32)
        q_off, cand_off = _c(q_off, np.uint64), _c(cand_off, np.uint64)
        nq = len(q_off) - 1
        at = out if out is not None else np.zeros(int(cand_off[-1]) if len(cand_off) else 0, np.uint32)
        self._check(self.L.sina_hip_find_bases(self.h, _ptr(qmask, u8p), _ptr(q_off, u64p), nq, _ptr(cand_ids, u32p), _ptr(cand_off, u64p),
                                               _ptr(at, u32p)))
        return at

    def find_bases_stats(self):
        """The containment kernel on this context so far: dict(kernel_ms, pairs, ref_bases, launches)."""
        return self._counters(self.L.sina_hip_find_bases_stats, KERNEL_MS + u64_fields("pairs", "ref_bases", "launches"))

    def count_pairs(self, on=True):
        """The switch of the in-place pair count: with it on, an align call with assemble=1 on a store with a helix map
        also counts the helix base pairs of every query it assembles (staged_pair_counts).  Off after init and fork."""
        self._check(self.L.sina_hip_align_count_pairs(self.h, 1 if on else 0))

    def staged_pair_counts(self):
        """uint32 [nq, 6] = num, AG, AU, CG, GG, GU of this context's last align call (a copy), rows laid out like its
        `out`: a query's counters where out[q].assembled == 1, six zeros elsewhere.  None if that call counted nothing
        (switch off, no helix map, assemble=0)."""
        p = self.L.sina_hip_staged_pair_counts(self.h)
        if not p:
            return None
        nq = getattr(self, "_align_nq", 0)
        return np.ctypeslib.as_array(p, shape=(max(nq, 1), 6))[:nq].copy()

    def pair_inplace_stats(self):
        """The in-place pair-count kernel on this context so far: dict(kernel_ms, sequences, launches); sequences
        counts assembled queries only."""
        return self._counters(self.L.sina_hip_pair_inplace_stats, KERNEL_MS + u64_fields("sequences", "launches"))

    def staged_shift_log(self):
        """The shifted runs of this context's last align call (assemble=2): a list with one entry per query, laid out
        like the call's `out` -- the query's events [(N, B, E), ...] in sequence order, the numbers of the reference's
        "shifting bases to fit in N bases at pos B to E;".  None unless that call ran with assemble=2."""
        p = self.L.sina_hip_staged_shift_log(self.h)
        if not p:
            return None
        nq = getattr(self, "_align_nq", 0)
        rows = np.ctypeslib.as_array(p, shape=(max(nq, 1), 1 + 3 * SHIFT_LOG))[:nq]
        return [[tuple(int(x) for x in r[1 + 3 * e:4 + 3 * e]) for e in range(int(r[0]))] for r in rows]

    def assemble_stats(self):
        """The device assembly on this context so far: dict(queries, assembled, shifted_queries, shifted_runs) over the
        fast path's launches that ran with assemble != 0."""
        return self._counters(self.L.sina_hip_assemble_stats, u64_fields("queries", "assembled", "shifted_queries", "shifted_runs"))

    def debug_assemble(self, params, width, qmask, qoff, out, out_pos):
        """The assembly alone on caller-made columns: out (ALIGN_OUT_DTYPE, with n_out, end_s, cutoff_head, cutoff_tail,
        aligned_bases, status) and out_pos (the columns as handed to cseq::append, laid out by qoff) come back as
        after an align call with `params` (assemble 1 or 2), as copies; the shift log is staged."""
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        out = np.array(out, ALIGN_OUT_DTYPE, copy=True)
        pos = np.array(out_pos, np.uint32, copy=True)
        assert len(out) == len(qoff) - 1 and len(pos) >= int(qoff[-1]) and len(qmask) >= int(qoff[-1])
        self._align_nq = len(qoff) - 1
        self._check(self.L.sina_hip_debug_assemble(self.h, C.byref(params), width, _ptr(qmask, u8p), _ptr(qoff, u64p), len(out),
                                                   out.ctypes.data_as(C.POINTER(AlignOut)), _ptr(pos, u32p)))
        return out, pos

    def debug_assemble_ms(self):
        """The assembly kernel's own time in this context's last debug_assemble call, in milliseconds."""
        return self._counters(self.L.sina_hip_debug_assemble_ms, KERNEL_MS)["kernel_ms"]

    def count_identity(self, on=True):
        """The switch of the in-place family identity (--calc-idty): with it on, align_families, align_families_wsets
        and align_profiles with assemble=1 also score every query they assemble against its family's members
        (staged_identity).  Off after init and fork."""
        self._check(self.L.sina_hip_align_count_identity(self.h, 1 if on else 0))

    def staged_identity(self):
        """uint32 [nq, 2] of this context's last align call (a copy), rows laid out like its `out`: the float bits of the
        best overlap score of the query with a member of its family and the number of members that have a score where
        out[q].assembled == 1, two zeros elsewhere.  None if that call counted nothing (switch off, assemble=0, an
        align_graphs call, no query)."""
        p = self.L.sina_hip_staged_identity(self.h)
        if not p:
            return None
        nq = getattr(self, "_align_nq", 0)
        return np.ctypeslib.as_array(p, shape=(max(nq, 1), 2))[:nq].copy()

    def identity_inplace_stats(self):
        """The in-place family-identity kernel on this context so far: dict(kernel_ms, sequences, pairs, launches);
        sequences counts assembled queries only, pairs their (query, member) pairs."""
        return self._counters(self.L.sina_hip_identity_inplace_stats, KERNEL_MS + u64_fields("sequences", "pairs", "launches"))

    def rank_assembled(self, on=True, k=10, nofast=False, kmer_candidates=1000, iupac=0, filter_lc=False, cover="query",
                       max_result=10):
        """The switch of the in-place ranking (the search stage where the device assembles): with it on, every fast-path
        align call with assemble != 0 on a store with a name order and an index of that k / nofast also searches its
        queries' k-mer candidates (kmer_candidates, at most 4096 after clamping to the references) and ranks them
        against every query it assembles without dropping a base (staged_rank).  The rules are compare_rank's.  Off
        after init and fork; a missing precondition leaves the align call as it is without the switch."""
        self._check(self.L.sina_hip_align_rank(self.h, 1 if on else 0, int(k), 1 if nofast else 0, int(kmer_candidates),
                                               int(iupac), int(filter_lc), self._cover(cover), int(max_result)))

    def staged_rank(self):
        """uint32 [nq, 130] of this context's last align call (a copy), rows laid out like its `out`: the number of rows
        n, the flags (bit 0: a candidate had a denominator of 0; bit 1: ranked), 64 ids, 64 score bit patterns, zero
        from n on -- kmer_topk_rank's rows for the same words.  A row the device did not rank is all zero.  None if
        that call did not rank (switch off, assemble=0, no index of the switch's k, no name order, no query)."""
        p = self.L.sina_hip_staged_rank(self.h)
        if not p:
            return None
        nq = getattr(self, "_align_nq", 0)
        return np.ctypeslib.as_array(p, shape=(max(nq, 1), RANK_ROW_WORDS))[:nq].copy()

    def rank_inplace_stats(self):
        """The in-place ranking kernel on this context so far: dict(kernel_ms, sequences, pairs, launches); sequences
        counts ranked queries, pairs their candidates, launches the DP launch ranges that ranked."""
        return self._counters(self.L.sina_hip_rank_inplace_stats, KERNEL_MS + u64_fields("sequences", "pairs", "launches"))

    def align_families(self, fam_ids, fam_off, qmask, qoff, params=None):
        params = params or self.params()
        fam_ids = _c(fam_ids, np.uint32)
        fam_off = _c(fam_off, np.uint64)
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        self._align_nq = len(qoff) - 1                  # (staged_pair_counts: rows of the last align call)
        nq = len(qoff) - 1
        out = np.zeros(nq, ALIGN_OUT_DTYPE)
        pos = np.zeros(max(len(qmask), 1), np.uint32)
        self._check(self.L.sina_hip_align_families(self.h, _ptr(fam_ids, u32p), _ptr(fam_off, u64p), nq,
                                                   _ptr(qmask, u8p), _ptr(qoff, u64p), C.byref(params),
                                                   out.ctypes.data_as(C.POINTER(AlignOut)), _ptr(pos, u32p)))
        return out, pos

    @staticmethod
    def params_wsets(weight_sets, **kw):
        """params() for the _wsets entries: weight_sets is [n_sets, n_weights], one positional weight vector per row."""
        ws = _c(weight_sets, np.float32)
        assert ws.ndim == 2 and ws.shape[0] >= 1
        p = Context.params(weights=ws.reshape(-1), **kw)
        p.n_weights = ws.shape[1]
        return p

    def align_graphs_wsets(self, gb, qmask, qoff, params, weight_set, n_sets):
        """align_graphs with a weight vector per query: params from params_wsets, weight_set[q] < n_sets (or None)."""
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        self._align_nq = len(qoff) - 1                  # (staged_pair_counts: rows of the last align call)
        ws = None if weight_set is None else _c(weight_set, np.uint32)
        out = np.zeros(gb.nq, ALIGN_OUT_DTYPE)
        pos = np.zeros(max(len(qmask), 1), np.uint32)
        self._check(self.L.sina_hip_align_graphs_wsets(self.h, C.byref(gb), _ptr(qmask, u8p), _ptr(qoff, u64p),
                                                       C.byref(params), None if ws is None else _ptr(ws, u32p), n_sets,
                                                       out.ctypes.data_as(C.POINTER(AlignOut)), _ptr(pos, u32p)))
        return out, pos

    def align_families_wsets(self, fam_ids, fam_off, qmask, qoff, params, weight_set, n_sets):
        """align_families with a weight vector per query (see align_graphs_wsets)."""
        fam_ids = _c(fam_ids, np.uint32)
        fam_off = _c(fam_off, np.uint64)
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        self._align_nq = len(qoff) - 1                  # (staged_pair_counts: rows of the last align call)
        ws = None if weight_set is None else _c(weight_set, np.uint32)
        nq = len(qoff) - 1
        out = np.zeros(nq, ALIGN_OUT_DTYPE)
        pos = np.zeros(max(len(qmask), 1), np.uint32)
        self._check(self.L.sina_hip_align_families_wsets(self.h, _ptr(fam_ids, u32p), _ptr(fam_off, u64p), nq,
                                                         _ptr(qmask, u8p), _ptr(qoff, u64p), C.byref(params),
                                                         None if ws is None else _ptr(ws, u32p), n_sets,
                                                         out.ctypes.data_as(C.POINTER(AlignOut)), _ptr(pos, u32p)))
        return out, pos

    def align_profiles(self, fam_ids, fam_off, qmask, qoff, params=None):
        """--fs-no-graph: like align_families, the families as profiles built on the device."""
        params = params or self.params()
        fam_ids = _c(fam_ids, np.uint32)
        fam_off = _c(fam_off, np.uint64)
        qmask = _c(qmask, np.uint8)
        qoff = _c(qoff, np.uint64)
        self._align_nq = len(qoff) - 1                  # (staged_pair_counts: rows of the last align call)
        nq = len(qoff) - 1
        out = np.zeros(nq, ALIGN_OUT_DTYPE)
        pos = np.zeros(max(len(qmask), 1), np.uint32)
        self._check(self.L.sina_hip_align_profiles(self.h, _ptr(fam_ids, u32p), _ptr(fam_off, u64p), nq,
                                                   _ptr(qmask, u8p), _ptr(qoff, u64p), C.byref(params),
                                                   out.ctypes.data_as(C.POINTER(AlignOut)), _ptr(pos, u32p)))
        return out, pos

    def debug_family_profile(self, fam_ids, match, mismatch, gap, gap_ext):
        """The profile the device builds for ONE family: (columns [n], match terms [n, 16], self terms [16]); the four
        numbers are the scheme's (-match_score, -mismatch_score, pen_gap, pen_gapext)."""
        fam_ids = _c(fam_ids, np.uint32)
        cap = 65536
        nn = C.c_uint32()
        pos = np.zeros(cap, np.uint32)
        sc = np.zeros((cap, 16), np.float32)
        own = np.zeros(16, np.float32)
        self._check(self.L.sina_hip_debug_family_profile(self.h, _ptr(fam_ids, u32p), len(fam_ids), match, mismatch, gap,
                                                         gap_ext, C.byref(nn), _ptr(pos, u32p), _ptr(sc, f32p),
                                                         _ptr(own, f32p), cap))
        return pos[:nn.value].copy(), sc[:nn.value].copy(), own

    def debug_family_profile_words(self, fam_ids):
        """The same build as the chain the DP kernel reads: dict(n, rec [n, 4] (the row records' words), succ_min [n],
        pred [n - 1] (the entries), sizes [8] (the size words)), all as they are on the device."""
        fam_ids = _c(fam_ids, np.uint32)
        cap = 65536
        nn = C.c_uint32()
        rec = np.zeros((cap, 4), np.uint32)
        smin = np.zeros(cap, np.uint32)
        pred = np.zeros(cap, np.uint32)
        sz = np.zeros(8, np.uint32)
        self._check(self.L.sina_hip_debug_family_profile_words(self.h, _ptr(fam_ids, u32p), len(fam_ids), C.byref(nn),
                                                               _ptr(rec, u32p), _ptr(smin, u32p), _ptr(pred, u32p),
                                                               _ptr(sz, u32p), cap))
        n = nn.value
        return dict(n=n, rec=rec[:n].copy(), succ_min=smin[:n].copy(), pred=pred[:max(n, 1) - 1].copy(), sizes=sz)

    def debug_mesh(self, gb, qmask, params=None, want_value=True, prune=False):
        """DP planes of ONE query.  prune=False (default): every row of every strip is swept, the planes are
        the reference's cell for cell; prune=True: the production launch with its certified row skip -- cells the
        kernel proved irrelevant hold whatever it left there (see dp_info / rgain for the bound it used)."""
        params = params or self.params()
        qmask = _c(qmask, np.uint8)
        n = int(gb._keep["node_off"][1])
        L = len(qmask)
        vm = np.zeros((n, L), np.uint32)
        vs = np.zeros((n, L), np.uint32)
        val = np.zeros((n, L), np.float32) if want_value else None
        self._check(self.L.sina_hip_debug_mesh(self.h, C.byref(gb), _ptr(qmask, u8p), L, C.byref(params),
                                               _ptr(vm, u32p), _ptr(vs, u32p),
                                               _ptr(val, f32p) if want_value else None, 1 if prune else 0))
        return vm, vs, val

    def debug_family_graph(self, fam_ids, fs_weight=1.0, ring_depth=4):
        fam_ids = _c(fam_ids, np.uint32)
        cap_n, cap_e = 65536, 400000
        nn, ne = C.c_uint32(), C.c_uint32()
        pos = np.zeros(cap_n, np.uint32)
        mask = np.zeros(cap_n, np.uint8)
        w = np.zeros(cap_n, np.float32)
        poff = np.zeros(cap_n + 1, np.uint32)
        pred = np.zeros(cap_e, np.uint32)
        smin = np.zeros(cap_n, np.uint32)
        sink = np.zeros(cap_n, np.uint8)
        spill = np.zeros(cap_n, np.uint32)
        self._check(self.L.sina_hip_debug_family_graph(self.h, _ptr(fam_ids, u32p), len(fam_ids), fs_weight,
                                                       ring_depth, C.byref(nn), C.byref(ne), _ptr(pos, u32p),
                                                       _ptr(mask, u8p), _ptr(w, f32p), _ptr(poff, u32p),
                                                       _ptr(pred, u32p), _ptr(smin, u32p), _ptr(sink, u8p),
                                                       _ptr(spill, u32p), cap_n, cap_e))
        n, e = nn.value, ne.value
        return dict(n=n, pos=pos[:n].copy(), mask=mask[:n].copy(), weight=w[:n].copy(), pred_off=poff[:n + 1].copy(),
                    pred=pred[:e].copy(), succ_minpos=smin[:n].copy(), sink=sink[:n].copy(), spill=spill[:n].copy())

    def debug_family_graph_words(self, fam_ids, fs_weight=1.0, ring_depth=4):
        """The same build as the words the DP kernel reads: dict(n, z, store (rec.w), pred (the entries, node by node),
        n_spill, first_sink, chain_len, status)."""
        fam_ids = _c(fam_ids, np.uint32)
        cap_n, cap_e = 65536, 400000
        nn, ne = C.c_uint32(), C.c_uint32()
        z = np.zeros(cap_n, np.uint32)
        w = np.zeros(cap_n, np.uint32)
        pred = np.zeros(cap_e, np.uint32)
        sz = np.zeros(8, np.uint32)
        self._check(self.L.sina_hip_debug_family_graph_words(self.h, _ptr(fam_ids, u32p), len(fam_ids), fs_weight,
                                                             ring_depth, C.byref(nn), C.byref(ne), _ptr(z, u32p),
                                                             _ptr(w, u32p), _ptr(pred, u32p), _ptr(sz, u32p), cap_n, cap_e))
        n, e = nn.value, ne.value
        return dict(n=int(sz[0]), z=z[:n].copy(), store=w[:n].copy(), pred=pred[:e].copy(), n_spill=int(sz[2]),
                    status=int(sz[3]), first_sink=int(sz[4]), gmin=int(sz[5]), chain_len=int(sz[6]))

    def dp_info(self, q=0):
        """What the DP kernel reported for query q of this context's last launch (row-skip test hook)."""
        d = DpInfo()
        self._check(self.L.sina_hip_debug_dp_info(self.h, q, C.byref(d)))
        return {f[0]: getattr(d, f[0]) for f in DpInfo._fields_}

    def rgain(self, n):
        """First n entries of the per-node row-skip bound the last launch / debug_family_graph left on the device:
        (R(m) in units of 1/64, C(m) = occupied columns right of the node's)."""
        out = np.zeros(max(n, 1), np.uint32)
        cols = np.zeros(max(n, 1), np.uint32)
        self._check(self.L.sina_hip_debug_rgain(self.h, n, _ptr(out, u32p), _ptr(cols, u32p)))
        return out[:n], cols[:n]

    def chain_rows(self):
        """The chain the last DAG build left for its first DAG: the node of every base of the family's first member."""
        cap = 65536
        out = np.zeros(cap, np.uint16)
        n = C.c_uint32()
        self._check(self.L.sina_hip_debug_chain_rows(self.h, out.ctypes.data_as(C.POINTER(C.c_uint16)), cap, C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def stats(self):
        s = Stats()
        self._check(self.L.sina_hip_get_stats(self.h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}
