"""ctypes binding of liborbfe.so (the gfx950 C-ABI declared in include/orbfe.h).

The library is built in-tree (make / __graft_entry__.build()) into pyorbslam_amd/_lib/.  There is no
CPU fallback: if the shared object is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

# ORBFE_LIB selects another in-tree build of the same C-ABI (same-box A/B of kernel revisions)
LIB_PATH = Path(os.environ.get("ORBFE_LIB") or Path(__file__).resolve().parent / "_lib" / "liborbfe.so")

ORBFE_OK = 0
ERRORS = {-1: "EINVAL", -2: "ENOMEM", -3: "EHIP", -4: "ECAPACITY", -5: "ESTATE", -6: "EOVERFLOW", -7: "EFORMAT",
          -8: "EREJECT"}
ORBFE_EINVAL = -1
ORBFE_ECAPACITY = -4
ORBFE_ESTATE = -5
ORBFE_EFORMAT = -7
ORBFE_EREJECT = -8


class Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("resize_simd_lanes", C.c_int32)]


class BatchView(C.Structure):
    _fields_ = [("kp_cap", C.c_int32), ("n_images", C.c_int32), ("n_pairs", C.c_int32),
                ("kps", C.c_void_p), ("desc", C.c_void_p), ("count", C.c_void_p), ("u_right", C.c_void_p),
                ("depth", C.c_void_p), ("status", C.c_void_p), ("match_r", C.c_void_p), ("overflow", C.c_void_p)]


class VocabInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32),
                ("n_nodes", C.c_int64), ("n_words", C.c_int64), ("depth", C.c_int32), ("max_children", C.c_int32)]


class VocabTrainParams(C.Structure):
    """orbfe_vocab_train_params."""
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32),
                ("max_iter", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


ORBFE_VOCAB_TRAIN_MAX_L = 10
VOCAB_TRAIN_DEPTH_COUNTERS = ("nodes_split", "iter_sum", "iter_max", "capped", "empty_dropped", "short_seeded")


class VocabTrainStats(C.Structure):
    """orbfe_vocab_train_stats: entry d of a per-depth array describes the nodes of depth d that were split."""
    _fields_ = ([("n_desc", C.c_int64), ("n_nodes", C.c_int64), ("n_words", C.c_int64)] +
                [(k, C.c_int64 * ORBFE_VOCAB_TRAIN_MAX_L) for k in VOCAB_TRAIN_DEPTH_COUNTERS] +
                [("depth_ms", C.c_double * ORBFE_VOCAB_TRAIN_MAX_L), ("weight_ms", C.c_double),
                 ("kernel_ms", C.c_double)])


ORBFE_ABI_VERSION = 9
ORBFE_BOW_MAX_FRAME = 8192  # the longest frame k_bow_assemble takes (include/orbfe.h)
# flags of BowOut.status
ORBFE_BOW_OVER_OUT, ORBFE_BOW_OVER_MAX, ORBFE_BOW_OVER_FRAME, ORBFE_BOW_NEGATIVE = 1, 2, 4, 8


class BowOut(C.Structure):
    """orbfe_bow_out: caller-owned output arrays of orbfe_vocab_bow / orbfe_vocab_bow_device."""
    _fields_ = [(k, C.c_void_p) for k in ("n_words", "bow_word", "bow_weight", "n_nodes", "fv_node", "fv_end",
                                          "fv_idx", "n_kept", "status")]


ORBFE_BOW_BAD_PAIR = 16  # orbfe_bow_match_device: a pair named a frame that does not exist


class BowMatchOut(C.Structure):
    """orbfe_bow_match_out: caller-owned output arrays of orbfe_bow_match / orbfe_bow_match_device."""
    _fields_ = [(k, C.c_void_p) for k in ("match12", "match21", "bin12", "hist", "n_raw", "status")]


ORBFE_TRI_ELIGIBLE, ORBFE_TRI_STEREO = 1, 2  # flag bits of orbfe_tri_match's per-feature byte
ORBFE_TRI_MARGINAL = 1  # orbfe_tri_match status: a decision of the pair lies within rounding of its threshold


class TriMatchOut(C.Structure):
    """orbfe_tri_match_out: caller-owned output arrays of orbfe_tri_match."""
    _fields_ = [(k, C.c_void_p) for k in ("match12", "bin12", "hist", "n_raw", "status", "stopped")]


ORBFE_FUSE_MARGINAL = 1  # orbfe_fuse_search status: a decision of the item lies within rounding of its threshold
ORBFE_FUSE_KF_F64, ORBFE_FUSE_PT_F64, ORBFE_FUSE_CHUNK = 27, 9, 256
ORBFE_SIM3_F64 = 28  # doubles per search of orbfe_sim3_search


class FuseOut(C.Structure):
    """orbfe_fuse_out: caller-owned output arrays of orbfe_fuse_search."""
    _fields_ = [(k, C.c_void_p) for k in ("best_idx", "best_dist", "status")]


class ScwOut(C.Structure):
    """orbfe_scw_out: caller-owned output arrays of orbfe_scw_search."""
    _fields_ = [(k, C.c_void_p) for k in ("best_idx", "best_dist", "status")]


class Sim3Out(C.Structure):
    """orbfe_sim3_out: caller-owned output arrays of orbfe_sim3_search, flat over the items."""
    _fields_ = [(k, C.c_void_p) for k in ("best_idx", "best_dist", "status")]


class FkfOut(C.Structure):
    """orbfe_fkf_out: caller-owned output arrays of orbfe_fkf_search, flat over the items."""
    _fields_ = [(k, C.c_void_p) for k in ("best_idx", "best_dist", "status")]


class LocalOut(C.Structure):
    """orbfe_local_out: caller-owned output arrays of orbfe_local_search, flat over the items."""
    _fields_ = [(k, C.c_void_p) for k in ("in_view", "level", "best_idx", "best_dist", "second_idx", "second_dist",
                                          "status")]


class FfOut(C.Structure):
    """orbfe_ff_out: caller-owned output arrays of orbfe_ff_search, flat over the items."""
    _fields_ = [(k, C.c_void_p) for k in ("best_idx", "best_dist", "status")]


class KfdbManyOut(C.Structure):
    """orbfe_kfdb_many_out: caller-owned host arrays of orbfe_kfdb_query_many / _many_device."""
    _fields_ = [(k, C.c_void_p) for k in ("n_sharing", "max_common", "n_hits", "hit_slot", "hit_common", "hit_first",
                                          "hit_score", "common", "first", "score")]


# cv::KeyPoint tuple layout (opencv_type_casters.h:106-108)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4")])

# every symbol include/orbfe.h declares (tests check the export table against the header)
SIGNATURES = {
    "orbfe_create": [C.POINTER(Params), C.POINTER(C.c_void_p)],
    "orbfe_destroy": [C.c_void_p],
    "orbfe_last_error": [],
    "orbfe_version": [],
    "orbfe_build_id": [],
    "orbfe_get_scales": [C.c_void_p] + [C.c_void_p] * 5,
    "orbfe_extract": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                      C.POINTER(C.c_int32)],
    "orbfe_pyramid": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "orbfe_stereo_match": [C.c_void_p, C.c_void_p, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_int32],
    "orbfe_frame_extract": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_float,
                            C.c_int32],
    "orbfe_frame_fetch": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
    "orbfe_frame_fetch_stereo": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.POINTER(C.c_int32)],
    "orbfe_frame_pyramid": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "orbfe_frame_serial": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "orbfe_frame_pyramid_fetch": [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64],
    "orbfe_undistort_points": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                               C.c_void_p],
    "orbfe_png_decode": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "orbfe_png_read_batch": [C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32],
    "orbfe_batch_reserve": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32],
    "orbfe_extract_batch_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p],
    "orbfe_stereo_batch_device": [C.c_void_p, C.c_int32, C.c_double, C.c_float, C.c_void_p],
    "orbfe_frontend_batch_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_float, C.c_void_p],
    "orbfe_batch_view_get": [C.c_void_p, C.POINTER(BatchView)],
    "orbfe_batch_status": [C.c_void_p, C.POINTER(C.c_int32)],
    "orbfe_batch_record_bytes": [C.c_void_p, C.POINTER(C.c_int64)],
    "orbfe_batch_pack_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p],
    "orbfe_batch_compact_record_bytes": [C.c_void_p, C.POINTER(C.c_int64)],
    "orbfe_batch_pack_compact_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p],
    "orbfe_batch_fetch": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
    "orbfe_batch_fetch_stereo": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.POINTER(C.c_int32)],
    "orbfe_hamming_search": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "orbfe_hamming_csr": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                          C.c_void_p],
    "orbfe_descriptor_distance": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)],
    "orbfe_grid_query": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                         C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_void_p, C.c_int64],
    "orbfe_select_f_f": [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p],
    "orbfe_select_f_p": [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p],
    "orbfe_hamming_matrix": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "orbfe_profile_begin": [C.c_void_p, C.c_int32],
    "orbfe_profile_read": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)],
    "orbfe_microbench": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)],
    "orbfe_debug_candidates": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
    "orbfe_debug_selected": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
    "orbfe_debug_octree_profile": [C.c_void_p, C.c_void_p, C.c_int64],
    "orbfe_debug_cascade_profile": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "orbfe_set_lanes": [C.c_void_p, C.c_int32],
    "orbfe_abi_version": [],
    "orbfe_set_graphs": [C.c_void_p, C.c_int32],
    "orbfe_graph_stats": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)],
    "orbfe_set_octree_kernel": [C.c_void_p, C.c_int32],
    "orbfe_get_octree_kernel": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
    "orbfe_get_stereo_bucket_kernel": [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "orbfe_debug_detect_stats": [C.c_void_p, C.POINTER(C.c_int64)],
    "orbfe_debug_detect_lanes": [C.c_void_p, C.POINTER(C.c_int64), C.c_int32],
    "orbfe_vocab_load_text": [C.c_char_p, C.POINTER(C.c_void_p)],
    "orbfe_vocab_create": [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.POINTER(C.c_void_p)],
    "orbfe_vocab_destroy": [C.c_void_p],
    "orbfe_vocab_get_info": [C.c_void_p, C.POINTER(VocabInfo)],
    "orbfe_vocab_get_nodes": [C.c_void_p] * 6,
    "orbfe_vocab_transform": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "orbfe_vocab_transform_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p],
    "orbfe_vocab_last_ms": [C.c_void_p, C.POINTER(C.c_float)],
    "orbfe_vocab_bow_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                               C.c_int64, C.POINTER(BowOut), C.c_void_p, C.c_int64, C.c_void_p],
    "orbfe_vocab_bow_scratch_bytes": [C.c_int32, C.c_int64, C.POINTER(C.c_int64)],
    "orbfe_vocab_bow": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(BowOut)],
    "orbfe_vocab_bow_last_ms": [C.c_void_p, C.POINTER(C.c_float)],
    "orbfe_vocab_train": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(VocabTrainParams),
                          C.POINTER(C.c_void_p), C.POINTER(VocabTrainStats)],
    "orbfe_vocab_save_text": [C.c_void_p, C.c_char_p],
    "orbfe_kfdb_create": [C.c_int64, C.c_int64, C.POINTER(C.c_void_p)],
    "orbfe_kfdb_destroy": [C.c_void_p],
    "orbfe_kfdb_add": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)],
    "orbfe_kfdb_erase": [C.c_void_p, C.c_int64],
    "orbfe_kfdb_clear": [C.c_void_p],
    "orbfe_kfdb_stats": [C.c_void_p] + [C.POINTER(C.c_int64)] * 6,
    "orbfe_kfdb_query": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_int64],
    "orbfe_bow_score": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                        C.c_void_p, C.c_void_p],
    "orbfe_kfdb_last_ms": [C.c_void_p, C.POINTER(C.c_float)],
    "orbfe_kfdb_query_many": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                              C.c_double, C.c_int32, C.c_int64, C.POINTER(KfdbManyOut)],
    "orbfe_kfdb_query_many_device": [C.c_void_p, C.POINTER(BowOut), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_double, C.c_int32, C.c_int64, C.POINTER(KfdbManyOut), C.c_void_p],
    "orbfe_kfdb_set_scratch_limit": [C.c_void_p, C.c_int64],
    "orbfe_kfdb_many_last_ms": [C.c_void_p, C.POINTER(C.c_float)],
    "orbfe_bow_match_device": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(BowOut), C.c_int64, C.c_void_p,
                               C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(BowMatchOut), C.c_int64,
                               C.c_void_p],
    "orbfe_bow_match": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                        C.POINTER(BowMatchOut), C.c_int64],
    "orbfe_bow_match_last_ms": [C.POINTER(C.c_float)],
    "orbfe_tri_match": [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 10 + [C.c_int32, C.c_int32, C.c_int32,
                                                                            C.POINTER(TriMatchOut), C.c_int64],
    "orbfe_tri_match_last_ms": [C.POINTER(C.c_float)],
    "orbfe_fuse_search": [C.c_void_p] * 14 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                              C.POINTER(FuseOut), C.c_int64],
    "orbfe_fuse_search_last_ms": [C.POINTER(C.c_float)],
    "orbfe_scw_search": [C.c_void_p] * 13 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                             C.POINTER(ScwOut), C.c_int64],
    "orbfe_scw_search_last_ms": [C.POINTER(C.c_float)],
    "orbfe_sim3_search": [C.c_void_p] * 12 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double,
                                              C.POINTER(Sim3Out)],
    "orbfe_sim3_search_last_ms": [C.POINTER(C.c_float)],
    "orbfe_fkf_search": [C.c_void_p] * 13 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_double, C.c_double, C.POINTER(FkfOut)],
    "orbfe_fkf_search_last_ms": [C.POINTER(C.c_float)],
    "orbfe_local_search": [C.c_void_p] * 14 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_int32, C.c_double,
                                               C.POINTER(LocalOut)],
    "orbfe_local_search_last_ms": [C.POINTER(C.c_float)],
    "orbfe_ff_search": [C.c_void_p] * 14 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                            C.POINTER(FfOut)],
    "orbfe_ff_search_last_ms": [C.POINTER(C.c_float)],
}

_lib: C.CDLL | None = None


class OrbfeError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed: {ERRORS.get(code, code)}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    """Load liborbfe.so (raises OSError if it is missing: no fallback path exists)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OSError(f"{LIB_PATH} not built: run `make` (or __graft_entry__.build()) first; "
                          "pyorbslam_amd has no CPU fallback")
        L = C.CDLL(str(LIB_PATH))
        for name, argtypes in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None and os.environ.get("ORBFE_LIB"):
                continue  # an older revision under A/B may predate some entry points
            if fn is None:
                raise OSError(f"{LIB_PATH} does not export {name}")
            fn.argtypes = argtypes
            fn.restype = C.c_char_p if name in ("orbfe_last_error", "orbfe_version", "orbfe_build_id") else C.c_int
        _lib = L
    return _lib


_pyhost = None


def pyhost():
    """The host-side CPython extension `_pyhost` (csrc/orbfe_pyhost.cpp): the per-frame Python objects of the
    reference data model (KeyPoint tuples, Frame.mGrid, mvuRight / mvDepth) built in C.  Raises ImportError
    when it is not built (`make`)."""
    global _pyhost
    if _pyhost is None:
        try:
            from . import _pyhost as m
        except ImportError as e:
            raise ImportError("pyorbslam_amd/_pyhost extension not built: run `make` (or __graft_entry__.build())") from e
        _pyhost = m
    return _pyhost


class OrbfeGeometryError(OrbfeError, ValueError):
    """A level geometry the reference's DistributeOctTree cannot take (vpIniNodes.resize of a negative nIni,
    ORBextractor.cpp:543-550): the reference throws std::length_error, which pybind11 raises as ValueError."""


def check(fn: str, rc: int) -> None:
    if rc != ORBFE_OK:
        msg = lib().orbfe_last_error().decode(errors="replace")
        if rc == -1 and "DistributeOctTree" in msg:  # EINVAL
            raise OrbfeGeometryError(fn, rc, msg)
        raise OrbfeError(fn, rc, msg)


def call(name: str, *args) -> None:
    check(name, getattr(lib(), name)(*args))


def has(name: str) -> bool:
    """Whether the loaded library exports `name` (always true for the in-tree build, which must export every
    declared symbol; an older build under ORBFE_LIB A/B may predate some)."""
    return getattr(lib(), name, None) is not None


def ptr(a: np.ndarray | None) -> C.c_void_p | None:
    return None if a is None else C.c_void_p(a.ctypes.data)


def make_params(nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int, minThFAST: int,
                resize_simd_lanes: int = 16) -> Params:
    # pybind11 narrows the scaleFactor argument to C++ float (orb_extractor.cpp:23)
    return Params(int(nfeatures), float(np.float32(scaleFactor)), int(nlevels), int(iniThFAST), int(minThFAST),
                  int(resize_simd_lanes))


def version() -> str:
    return lib().orbfe_version().decode()


def build_id() -> str:
    """SHA-256 prefix of the sources the loaded library was built from (orbfe_build_id)."""
    fn = getattr(lib(), "orbfe_build_id", None)
    return fn().decode() if fn is not None else "unknown"


_device_present: bool | None = None


def device_present() -> bool:
    """Whether the HIP runtime the library is linked against sees a device; asked once (hipGetDeviceCount, reached
    through the library's own dependency, so nothing else is loaded)."""
    global _device_present
    if _device_present is None:
        n = C.c_int(0)
        fn = getattr(lib(), "hipGetDeviceCount", None)
        _device_present = fn is not None and fn(C.byref(n)) == 0 and n.value > 0
    return _device_present


def gpu_available() -> bool:
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:  # pragma: no cover
        return False
