"""Drop-in for the reference ORBMatcher (ORBMatcher.py): every search of the class.

descriptor_distance (ORBMatcher.py:12-14), the BoW searches search_by_BoW_kf_f / _kf_kf (:21-213), the
projection searches search_by_projection_f_p / _f_f / _ckf_scw_mp / _f_kf_f (:215-393, 850-1008), the
fusions fuse_kf_scw_mp / fuse_pkf_mp (:395-582), search_for_triangulation (:584-711) and search_by_sim3
(:713-848) keep the reference's control flow and results exactly; what changes is where the popcounts
happen.  The reference calls a per-byte Python popcount (~10 us) once per
candidate inside the search loop.  Here every (query, candidate) pair of a search is collected first —
the candidate windows depend only on the frame grid, never on matches made during the search — and
all distances come back from ONE k_hamming_search launch (orbfe_hamming_csr).  The sequential part
that genuinely depends on earlier iterations (candidates already holding a map point with
observations, the stereo gate, best / second-best bookkeeping, the rotation histogram) then runs on the
host over those precomputed distances, evaluating the same Python expressions on the same objects, so
every dtype promotion of the reference is preserved.

The split into "collect, then replay" is exact because everything the collection phase evaluates is
static during a search (keypoints, grids, poses, map-point geometry, map-point badness at collection
time — badness never reverts), while every piece of state a search mutates (matched slots, keyframe
map-point slots, observations) is read in the replay phase at the reference's point in the loop.  The one
input a search can change under itself is a map point's descriptor (fuse_pkf_mp: MapPoint.replace
recomputes the survivor's distinctive descriptor, MapPoint.py:180); the replay compares the descriptor it
reads with the collected one and re-runs that query's distances on the GPU when they differ.

The replay loops restate ORBMatcher.py statement by statement on purpose: a drop-in must reproduce the
reference's control flow, NumPy-2 dtype promotions and the order of its side effects exactly, so those
lines necessarily read like the reference's.  The two tracking searches also have a native selection
(orbfe_select_f_f / _f_p, host C) used when every compared value is a double.

Three searches that the reference's callers run in a loop over candidates also exist for the whole list at
once, one kernel launch and no host replay: search_by_BoW_kf_kf_many / search_by_BoW_kf_f_many (k_bow_match) and
search_for_triangulation_many (k_tri_match).  Each returns what the loop of single searches returns; an element
the kernels' arrays cannot express, or whose float64 decision lies within rounding of its threshold, takes the
single search.  fuse_pkf_mp_many (k_fuse_search) does the same for LocalMapping's fusion loops: one launch for
the search of every (keyframe, point), then the matches applied on the host in the reference's order.
fuse_kf_scw_mp_many and search_by_projection_ckf_scw_mp (k_scw_search) do it for LoopClosing's two Sim3 searches,
and search_by_sim3 / search_by_sim3_many (k_sim3_search) for its mutual search: both directions of every candidate
pair in one launch, nothing to replay in order.  search_by_projection_f_kf_f / _f_kf_f_many (k_fkf_search) do it
for Tracking.relocalization's search into a frame, which assigns into the frame it searches: one launch, then the
assignments replayed in list order.  search_local_points / search_local_points_many (k_local_search) do it for
Tracking.search_local_points: Frame.is_in_frustum over the local map and search_by_projection_f_p in one launch, the
attributes written by frame.is_in_frustum_many on the host, the assignments replayed in list order.
"""
from __future__ import annotations

import ctypes as C
import operator
import threading
import weakref
from collections import deque
from itertools import compress, repeat

import numpy as np

from . import _lib
from ._lib import call, ptr

TH_HIGH = 100     # ORBMatcher.py:3
TH_LOW = 50       # ORBMatcher.py:4
HISTO_LENGTH = 30  # ORBMatcher.py:5


class _OwnedHandle:
    """An orbfe handle (own stream + Hamming scratch) destroyed with its owner."""

    def __init__(self):
        self.h = C.c_void_p()
        call("orbfe_create", C.byref(_lib.make_params(2000, 1.2, 8, 20, 7)), C.byref(self.h))

    def __del__(self):
        if self.h.value and _lib._lib is not None:
            _lib.lib().orbfe_destroy(self.h)
            self.h = C.c_void_p()


# One handle per calling thread: the reference runs Tracking, LocalMapping and LoopClosing as threads
# that all use ORBMatcher and MapPoint (System.py:59-64).  A thread's handle is destroyed with its
# thread-local storage; the C side also serialises the Hamming calls of one handle (orbfe_ctx::hmu).
_local = threading.local()


def _h():
    o = getattr(_local, "owned", None)
    if o is None:
        o = _local.owned = _OwnedHandle()
    return o.h


def hamming_csr(queries: np.ndarray, train: np.ndarray, cand_off: np.ndarray, cand_idx: np.ndarray) -> np.ndarray:
    """popcount(queries[q] ^ train[cand_idx[k]]) for k in [cand_off[q], cand_off[q+1]), on the GPU."""
    q = np.ascontiguousarray(queries, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
    off = np.ascontiguousarray(cand_off, np.int32)
    idx = np.ascontiguousarray(cand_idx, np.int32)
    out = np.empty(max(int(off[-1]) if len(off) else 0, 1), np.int32)
    if len(q) == 0 or off[-1] == 0:
        return out[:0]
    call("orbfe_hamming_csr", _h(), ptr(q), len(q), ptr(t), len(t), ptr(off), ptr(idx), ptr(out))
    return out[:int(off[-1])]


def descriptor_distance(a, b) -> int:
    """popcount(a ^ b) of two 32-byte descriptors (liborbfe host popcount: one pair does not pay a device
    round trip)."""
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    if a.size != 32 or b.size != 32:
        raise ValueError("descriptors must be 32 bytes")
    out = C.c_int32()
    _lib.check("orbfe_descriptor_distance", _lib.lib().orbfe_descriptor_distance(a.ctypes.data, b.ctypes.data,
                                                                               C.byref(out)))
    return out.value


def hamming_matrix(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
    out = np.zeros((len(a), len(b)), np.int32)
    if len(a) and len(b):
        call("orbfe_hamming_matrix", _h(), ptr(a), len(a), ptr(b), len(b), ptr(out))
    return out


# ---------------------------------------------------------------------------------------- grid queries
# Frame.get_features_in_area (Frame.py:373-416) for all the queries of a search at once (orbfe_grid_query,
# host code in liborbfe).  Used when every operand is a double (Python float, np.float64, or a 1-element
# float64 array — the types the reference's tracking loop produces); any other operand type (a float32
# projection evaluates in float32 under NumPy 2's promotion rules) goes through the frame's own method.
_grid_cache = weakref.WeakKeyDictionary()
_F64 = (float, np.float64)


def _is_f64(v) -> bool:
    return type(v) in _F64 or (type(v) is np.ndarray and v.dtype == np.float64 and v.size == 1)


_DTYPE, _SIZE, _SHAPE = operator.attrgetter("dtype"), operator.attrgetter("size"), operator.attrgetter("shape")
_F64_DT = np.dtype(np.float64)


def _f64_array(vals: list):
    """vals as a float64 array when every element is a double in _is_f64's sense (Python float, np.float64, or
    a size-1 float64 ndarray: the values are taken exactly), else None.  The type checks run as map() over
    C-level callables, not per element in Python (the tracking searches pass ~1 000 projections each)."""
    n = len(vals)
    if n == 0:
        return np.zeros(0, np.float64)
    kinds = set(map(type, vals))
    if kinds <= _F64_SET:
        return np.array(vals, np.float64)
    if kinds == _NDARRAY_SET and set(map(_DTYPE, vals)) == {_F64_DT} and set(map(_SIZE, vals)) == {1}:
        if len(set(map(_SHAPE, vals))) == 1:  # one shape: a single (n, 1[, 1]) float64 array
            return np.array(vals, np.float64).reshape(n)
        return np.fromiter((v.item() for v in vals), np.float64, count=n)
    if all(_is_f64(v) for v in vals):  # a mix of the kinds above
        return np.fromiter((v.item() if type(v) is np.ndarray else v for v in vals), np.float64, count=n)
    return None


_F64_SET = frozenset(_F64)
_NDARRAY_SET = frozenset((np.ndarray,))
_INT_SET = frozenset((int, np.int64, np.int32))
_U8_DT = np.dtype(np.uint8)
_UR_SET = frozenset((int, float, np.float32, np.float64))
_DOUBLE_OR_INT_SET = frozenset((float, int, np.float64))
_ANGLE = operator.attrgetter("angle")
_OBSERVATIONS = operator.methodcaller("observations")
_OCTAVE = operator.attrgetter("octave")
_IN_VIEW = operator.attrgetter("mbTrackInView")
_IS_BAD = operator.methodcaller("is_bad")
_VIEW_COS = operator.attrgetter("mTrackViewCos")
_TRACK_LEVEL = operator.attrgetter("mnTrackScaleLevel")
_PROJ_X = operator.attrgetter("mTrackProjX")
_PROJ_Y = operator.attrgetter("mTrackProjY")
_PROJ_XR = operator.attrgetter("mTrackProjXR")
_WORLD_POS = operator.methodcaller("get_world_pos")
_DESCRIPTOR = operator.methodcaller("get_descriptor")


def _frame_grid(frame):
    """(cell_off, cell_idx, kp_x, kp_y, kp_oct, frame4) of a frame, cached while its grid / keypoints are
    the same objects; None if the frame's grid parameters are not plain doubles."""
    try:
        ent = _grid_cache.get(frame)
    except TypeError:
        return None
    key = (id(frame.mGrid), id(frame.mvKeysUn), frame.N)
    if ent is not None and ent[0] == key:
        return ent[1]
    f4 = (frame.mnMinX, frame.mnMinY, frame.mfGridElementWidthInv, frame.mfGridElementHeightInv)
    if not all(type(v) in _F64 for v in f4):
        return None
    cols, rows = frame.FRAME_GRID_COLS, frame.FRAME_GRID_ROWS
    csr = getattr(frame, "_orbfe_grid", None)  # left by frame.assign_features_to_grid for this mGrid
    if csr is not None and csr[0] == id(frame.mGrid) and len(csr[1]) == cols * rows + 1:
        off, idx = csr[1], csr[2]
    else:
        sizes = np.fromiter((len(frame.mGrid[ix][iy]) for ix in range(cols) for iy in range(rows)), np.int32,
                            count=cols * rows)
        off = np.zeros(cols * rows + 1, np.int32)
        np.cumsum(sizes, out=off[1:])
        idx = np.fromiter((g for col in frame.mGrid for cell in col for g in cell), np.int32, count=int(off[-1]))
    kps = frame.mvKeysUn
    pts = getattr(frame, "_orbfe_pts", None)  # left by frame.assign_features_to_grid: (mvKeys, (N, 2) f64)
    if pts is not None and pts[0] is kps and kps is frame.mvKeys and len(pts[1]) == len(kps):
        kx, ky = np.ascontiguousarray(pts[1][:, 0]), np.ascontiguousarray(pts[1][:, 1])
        ko = _octaves(frame)
    else:
        kx = np.fromiter((k.pt[0] for k in kps), np.float64, count=len(kps))
        ky = np.fromiter((k.pt[1] for k in kps), np.float64, count=len(kps))
        ko = np.fromiter((k.octave for k in kps), np.int32, count=len(kps))
    grid = (off, idx, kx, ky, ko, np.array(f4, np.float64), cols, rows)
    _grid_cache[frame] = (key, grid)
    return grid


_octave_cache = weakref.WeakKeyDictionary()


def _octaves(frame) -> np.ndarray:
    """frame.mvKeys[i].octave as an int32 array, cached while mvKeys is the same list of the same length."""
    kps = frame.mvKeys
    key = (id(kps), len(kps))
    try:
        ent = _octave_cache.get(frame)
    except TypeError:
        ent = None
    if ent is not None and ent[0] == key:
        return ent[1]
    kxy = getattr(frame, "_orbfe_kxy", None)  # frame.extract_orb's copy of the fields mvKeys was built from
    if kxy is not None and kxy[0] is kps and len(kxy[2]) == len(kps) and _kp_field_ok(kps, kxy[2], "octave", int):
        arr = kxy[2]
    else:
        arr = np.fromiter((k.octave for k in kps), np.int32, count=len(kps))
    try:
        _octave_cache[frame] = (key, arr)
    except TypeError:
        pass
    return arr


_angle_cache = weakref.WeakKeyDictionary()


def _kp_field_ok(kps, arr, name, typ) -> bool:
    """The KeyPoint class kept the extractor's values as given (spot check of the first and last keypoint:
    the type and the value of field `name`), so the extractor's array stands for the KeyPoints' fields."""
    if len(kps) == 0:
        return True
    a, b = getattr(kps[0], name), getattr(kps[-1], name)
    return type(a) is typ and type(b) is typ and a == arr[0] and b == arr[-1]


def _angles(frame):
    """mvKeysUn[i].angle as doubles (the rotation histogram's input), cached per keypoint list; None when
    an angle is not a double (a float32 angle would make the reference's subtraction float32)."""
    kps = frame.mvKeysUn
    key = (id(kps), len(kps))
    try:
        ent = _angle_cache.get(frame)
    except TypeError:
        ent = None
    if ent is not None and ent[0] == key:
        return ent[1]
    arr = None
    kxy = getattr(frame, "_orbfe_kxy", None)
    if kxy is not None and kxy[0] is kps and len(kxy[3]) == len(kps) and _kp_field_ok(kps, kxy[3], "angle", float):
        arr = kxy[3]  # the KeyPoints' angles are the Python floats of these float32 values
    else:
        angles = list(map(_ANGLE, kps))
        if set(map(type, angles)) <= _F64_SET:
            arr = np.array(angles, np.float64)
    try:
        _angle_cache[frame] = (key, arr)
    except TypeError:
        pass
    return arr


def _grid_csr(frame, grid, qx, qy, qr, lo, hi):
    """orbfe_grid_query over float64 / int32 query arrays: (out_off, out_idx) as int32 arrays."""
    off, idx, kx, ky, ko, f4, cols, rows = grid
    qx, qy, qr = (np.ascontiguousarray(a, np.float64) for a in (qx, qy, qr))
    lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
    n = len(qx)
    out_off = np.zeros(n + 1, np.int32)
    cap = max(64 * n, 1)
    while True:
        out = np.empty(cap, np.int32)
        rc = _lib.lib().orbfe_grid_query(ptr(off), ptr(idx), cols, rows, ptr(kx), ptr(ky), ptr(ko), len(kx), ptr(f4), n,
                                         ptr(qx), ptr(qy), ptr(qr), ptr(lo), ptr(hi), ptr(out_off), ptr(out), cap)
        if rc == _lib.ORBFE_ECAPACITY:
            cap = int(out_off[-1])
            continue
        _lib.check("orbfe_grid_query", rc)
        return out_off, out[:int(out_off[-1])]


def features_in_areas(frame, queries) -> list:
    """[frame.get_features_in_area(x, y, r, lo, hi) for (x, y, r, lo, hi) in queries], batched."""
    if not queries:
        return []
    grid = _frame_grid(frame)
    fast = grid is not None and all(_is_f64(x) and _is_f64(y) and _is_f64(r) for x, y, r, _, _ in queries)
    if not fast:
        return [frame.get_features_in_area(*q) for q in queries]
    n = len(queries)
    qx = np.fromiter((q[0].item() if type(q[0]) is np.ndarray else q[0] for q in queries), np.float64, count=n)
    qy = np.fromiter((q[1].item() if type(q[1]) is np.ndarray else q[1] for q in queries), np.float64, count=n)
    qr = np.fromiter((q[2].item() if type(q[2]) is np.ndarray else q[2] for q in queries), np.float64, count=n)
    lo = np.fromiter((q[3] for q in queries), np.int32, count=n)
    hi = np.fromiter((q[4] for q in queries), np.int32, count=n)
    out_off, out = _grid_csr(frame, grid, qx, qy, qr, lo, hi)
    o = out_off.tolist()
    flat = out.tolist()
    return [flat[o[i]:o[i + 1]] for i in range(n)]


# Per-frame inputs of the native candidate selection: mvuRight as doubles (set once by the Frame
# constructor), and which slots hold a map point with observations (read fresh per search).
_uright_cache = weakref.WeakKeyDictionary()


def _u_right(frame, with_kinds: bool = False):
    """frame.mvuRight widened to a float64 array (cached while the list is the same object); with_kinds
    also returns whether every entry is already a double (Python float / int or np.float64), i.e. whether
    `python_float - mvuRight[i]` evaluates in double under NumPy 2's promotion rules (NEP 50: a Python
    float meeting an np.float32 stays float32)."""
    vals = frame.mvuRight
    try:
        ent = _uright_cache.get(frame)
    except TypeError:
        ent = None
    if ent is None or ent[0] != (id(vals), len(vals)):
        kinds = set(map(type, vals))
        if kinds <= _UR_SET:  # the values the drop-in's lists hold: -1, np.float32, Python float
            arr = np.array(vals, np.float64)  # each value widened exactly, as float(v)
        else:
            arr = np.fromiter((float(v) for v in vals), np.float64, count=len(vals))
        all_double = kinds <= _DOUBLE_OR_INT_SET
        ent = ((id(vals), len(vals)), arr, all_double)
        try:
            _uright_cache[frame] = ent
        except TypeError:
            pass
    return (ent[1], ent[2]) if with_kinds else ent[1]


def prime_u_right(frame, res: dict, xs: np.ndarray) -> None:
    """Fill _u_right's cache for a frame whose mvuRight list compute_stereo_matches has just built from the
    stereo arrays (frame.to_reference_lists): the same doubles, from the arrays instead of the 2 000-entry
    list — u_right widened where status is 1, -1 where 0, float(x) - 0.01 where 2 (Frame.py:273-277)."""
    vals = frame.mvuRight
    st = np.asarray(res["status"])
    if len(vals) != len(st):
        return
    arr = np.asarray(res["u_right"], np.float32).astype(np.float64)
    arr[st == 0] = -1.0
    z = st == 2
    if z.any():
        arr[z] = np.asarray(xs, np.float32)[z].astype(np.float64) - 0.01
    # np.float32 entries (status 1) are not doubles; -1 (int) and the status-2 Python floats are
    all_double = not bool(((st != 0) & (st != 2)).any())
    try:
        _uright_cache[frame] = ((id(vals), len(vals)), arr, all_double)
    except TypeError:
        pass


def _blocked(frame):
    """Per slot of the frame: 1 if it holds a map point with observations (ORBMatcher.py's
    `if mvpMapPoints[i]: if mvpMapPoints[i].observations() > 0: continue`)."""
    mps = frame.mvpMapPoints
    n = len(mps)
    out = np.zeros(n, np.uint8)
    if mps.count(None) == n:
        return out
    held = np.flatnonzero(np.fromiter(map(operator.is_not, mps, repeat(None, n)), bool, count=n))
    hl = held.tolist()
    out[held] = _obs_flags([mps[i] for i in hl])
    return out


def _obs_flags(mps) -> np.ndarray:
    """1 per map point that is truthy and has observations() > 0."""
    if all(mps):
        obs = list(map(_OBSERVATIONS, mps))
        if set(map(type, obs)) <= _INT_SET:
            return (np.array(obs, np.int64) > 0).astype(np.uint8)
    return np.fromiter((1 if (m and m.observations() > 0) else 0 for m in mps), np.uint8, count=len(mps))


def _descriptor_rows(descs: list) -> np.ndarray:
    """(n, 32) u8 array of n map-point descriptors (one array copy when they are all 32-byte u8 arrays)."""
    if (set(map(type, descs)) == _NDARRAY_SET and set(map(_DTYPE, descs)) == {_U8_DT}
            and set(map(_SIZE, descs)) == {32} and len(set(map(_SHAPE, descs))) == 1):
        return np.concatenate(descs).reshape(len(descs), 32)
    return np.stack([np.asarray(d, np.uint8).reshape(32) for d in descs])


def bow_match_arrays(desc, angle, off, fv_off, fv_node, fv_end, fv_idx, pairs, th=TH_LOW, inclusive=False,
                     nnratio=1.0, elig1=None, elig2=None) -> dict:
    """orbfe_bow_match (k_bow_match, include/orbfe.h): the BoW-guided match of ORBMatcher.py:21-213 for many frame
    pairs in one launch, before the rotation rejection.  Frame f is features [off[f], off[f + 1]) of desc (x 32
    u8) / angle (f32) / elig1 / elig2 (u8, None = all eligible), its feature vector nodes [fv_off[f], fv_off[f + 1])
    of fv_node / fv_end with the indices at fv_idx[off[f]:]; pairs: (P, 2) frame indices.  Returns match12,
    match21 (P, stride) int32, bin12 (P, stride) int8, hist (P, 32), n_raw (P,) and status; row p holds n1 / n2
    entries, the rest stays -1."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)
    desc, angle = arr(desc, np.uint8), arr(angle, np.float32)
    off, fv_off = arr(off, np.int64), arr(fv_off, np.int64)
    fv_node, fv_end, fv_idx = arr(fv_node, np.int32), arr(fv_end, np.int32), arr(fv_idx, np.int32)
    elig1, elig2 = arr(elig1, np.uint8), arr(elig2, np.uint8)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n_frames, n_pairs = max(len(off) - 1, 0), len(pairs)
    n = int(off[-1]) if n_frames > 0 else 0
    for a, per in ((desc, 32), (angle, 1), (elig1, 1), (elig2, 1), (fv_idx, 1)):
        if a is not None and a.size < n * per:
            raise ValueError("a per-feature array is shorter than off[-1] features")
    if n_frames > 0 and (len(fv_off) != n_frames + 1 or min(len(fv_node), len(fv_end)) < int(fv_off[-1])):
        raise ValueError("fv_off / fv_node / fv_end do not cover the frames")
    stride = int(np.diff(off).max()) if n_frames > 0 else 0
    m12 = np.full((n_pairs, stride), -1, np.int32)
    m21 = np.full((n_pairs, stride), -1, np.int32)
    b12 = np.full((n_pairs, stride), -1, np.int8)
    hist = np.zeros((n_pairs, 32), np.int32)
    n_raw = np.zeros(n_pairs, np.int32)
    status = np.zeros(1, np.int32)
    out = _lib.BowMatchOut(match12=m12.ctypes.data, match21=m21.ctypes.data, bin12=b12.ctypes.data,
                           hist=hist.ctypes.data, n_raw=n_raw.ctypes.data, status=status.ctypes.data)
    call("orbfe_bow_match", ptr(desc), ptr(angle), ptr(elig1), ptr(elig2), ptr(off), n_frames, ptr(fv_off),
         ptr(fv_node), ptr(fv_end), ptr(fv_idx), ptr(pairs), n_pairs, int(th), int(bool(inclusive)), float(nnratio),
         C.byref(out), stride)
    return dict(match12=m12, match21=m21, bin12=b12, hist=hist, n_raw=n_raw, status=int(status[0]))


class _BowFrame:
    __slots__ = ("desc", "angle", "elig", "fv_node", "fv_end", "fv_idx")


def _bow_frame(obj, kps, vp):
    """Array form of a keyframe / frame for k_bow_match: descriptors, the angles of `kps` as float32, eligibility
    from the map-point list `vp` (None: every feature) and the feature vector as CSR.  None when the arrays cannot
    express the object (the caller then takes the single search): an angle that is not a double holding a float32
    value, feature-vector keys not ascending, an index outside the frame or in two runs, descriptors that are
    not n x 32 u8, a map-point list of another length, or a frame above the kernel's cap."""
    desc = np.asarray(obj.mDescriptors)
    if desc.ndim != 2 or desc.shape[1] != 32 or desc.dtype != _U8_DT:
        return None
    n = len(desc)
    if n > _lib.ORBFE_BOW_MAX_FRAME or len(kps) != n or (vp is not None and len(vp) != n):
        return None
    if kps is obj.mvKeysUn:
        ang = _angles(obj)
    else:
        vals = list(map(_ANGLE, kps))
        ang = np.array(vals, np.float64) if set(map(type, vals)) <= _F64_SET else None
    if ang is None:
        return None
    a32 = ang.astype(np.float32)
    if not np.array_equal(a32.astype(np.float64), ang):
        return None
    fv = obj.mFeatVec
    nodes = list(fv)
    if not set(map(type, nodes)) <= _INT_SET or any(b <= a for a, b in zip(nodes, nodes[1:])):
        return None
    if nodes and not -2**31 <= nodes[0] <= nodes[-1] < 2**31:
        return None
    runs = [fv[k] for k in nodes]
    lens = np.fromiter(map(len, runs), np.int64, count=len(runs))
    try:
        idx = np.fromiter((i for r in runs for i in r), np.int64, count=int(lens.sum()))
    except (TypeError, ValueError):
        return None
    if len(idx) and (idx.min() < 0 or idx.max() >= n or len(np.unique(idx)) != len(idx)):
        return None
    f = _BowFrame()
    f.desc, f.angle = desc, a32
    if vp is None:
        f.elig = np.ones(n, np.uint8)
    else:
        f.elig = np.fromiter((1 if p and not p.is_bad() else 0 for p in vp), np.uint8, count=n)
    f.fv_node = np.array(nodes, np.int32)
    f.fv_end = np.cumsum(lens).astype(np.int32)
    f.fv_idx = idx.astype(np.int32)
    return f


def tri_match_arrays(desc, angle, xy, octave, flags, off, fv_off, fv_node, fv_end, fv_idx, lvl_off, thr_epi, thr_ex,
                     pairs, F12, epipole, th=TH_LOW, only_stereo=False) -> dict:
    """orbfe_tri_match (k_tri_match, include/orbfe.h): the match of ORBMatcher.search_for_triangulation
    (ORBMatcher.py:584-711) for many keyframe pairs in one launch, before the rotation rejection.  Frame f is
    features [off[f], off[f + 1]) of desc (x 32 u8) / angle (f32) / xy (x 2 f64) / octave (i32) / flags (u8:
    ORBFE_TRI_ELIGIBLE | ORBFE_TRI_STEREO), its feature vector nodes [fv_off[f], fv_off[f + 1]) of fv_node / fv_end
    with the indices at fv_idx[off[f]:], its levels [lvl_off[f], lvl_off[f + 1]) of thr_epi / thr_ex (f64); pairs:
    (P, 2) frame indices, F12 (P, 3, 3) f64, epipole (P, 2) f64.  Returns match12 (P, stride) int32, bin12
    (P, stride) int8, hist (P, 32), n_raw, status and stopped (P,); row p holds n1 entries, the rest stays -1."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)
    desc, angle, xy = arr(desc, np.uint8), arr(angle, np.float32), arr(xy, np.float64)
    octave, flags = arr(octave, np.int32), arr(flags, np.uint8)
    off, fv_off, lvl_off = arr(off, np.int64), arr(fv_off, np.int64), arr(lvl_off, np.int64)
    fv_node, fv_end, fv_idx = arr(fv_node, np.int32), arr(fv_end, np.int32), arr(fv_idx, np.int32)
    thr_epi, thr_ex = arr(thr_epi, np.float64), arr(thr_ex, np.float64)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    F12 = np.ascontiguousarray(F12, np.float64).reshape(-1, 9)
    epipole = np.ascontiguousarray(epipole, np.float64).reshape(-1, 2)
    n_frames, n_pairs = max(len(off) - 1, 0), len(pairs)
    if len(F12) != n_pairs or len(epipole) != n_pairs:
        raise ValueError("F12 / epipole do not cover the pairs")
    n = int(off[-1]) if n_frames > 0 else 0
    for a, per in ((desc, 32), (angle, 1), (xy, 2), (octave, 1), (flags, 1), (fv_idx, 1)):
        if a is not None and a.size < n * per:
            raise ValueError("a per-feature array is shorter than off[-1] features")
    if n_frames > 0 and (len(fv_off) != n_frames + 1 or min(len(fv_node), len(fv_end)) < int(fv_off[-1])):
        raise ValueError("fv_off / fv_node / fv_end do not cover the frames")
    if n_frames > 0 and (len(lvl_off) != n_frames + 1 or min(len(thr_epi), len(thr_ex)) < int(lvl_off[-1])):
        raise ValueError("lvl_off / thr_epi / thr_ex do not cover the frames")
    stride = int(np.diff(off).max()) if n_frames > 0 else 0
    m12 = np.full((n_pairs, stride), -1, np.int32)
    b12 = np.full((n_pairs, stride), -1, np.int8)
    hist = np.zeros((n_pairs, 32), np.int32)
    n_raw = np.zeros(n_pairs, np.int32)
    status = np.zeros(n_pairs, np.int32)
    stopped = np.zeros(n_pairs, np.int32)
    out = _lib.TriMatchOut(match12=m12.ctypes.data, bin12=b12.ctypes.data, hist=hist.ctypes.data,
                           n_raw=n_raw.ctypes.data, status=status.ctypes.data, stopped=stopped.ctypes.data)
    call("orbfe_tri_match", ptr(desc), ptr(angle), ptr(xy), ptr(octave), ptr(flags), ptr(off), n_frames, ptr(fv_off),
         ptr(fv_node), ptr(fv_end), ptr(fv_idx), ptr(lvl_off), ptr(thr_epi), ptr(thr_ex), ptr(pairs), ptr(F12),
         ptr(epipole), n_pairs, int(th), int(bool(only_stereo)), C.byref(out), stride)
    return dict(match12=m12, bin12=b12, hist=hist, n_raw=n_raw, status=status, stopped=stopped)


class _TriFrame:
    __slots__ = ("desc", "angle", "xy", "xy_f32", "octave", "flags", "fv_node", "fv_end", "fv_idx", "thr_epi",
                 "thr_ex")


def _tri_frame(kf):
    """Array form of a keyframe for k_tri_match: what _bow_frame gives for mvKeysUn, plus the undistorted
    positions and octaves, the flag byte (ORBFE_TRI_ELIGIBLE: the slot holds nothing truthy, as
    `not get_map_point(i)`; ORBFE_TRI_STEREO: mvuRight[i] >= 0) and the per-level thresholds
    3.84 * mvLevelSigma2[l] and 100 * mvScaleFactors[l], evaluated as the reference writes them and then widened.
    None when the arrays cannot express the keyframe (the caller then takes the single search): what _bow_frame
    refuses, a coordinate that is not a double, an octave outside the level tables, a threshold that is not
    finite, or lists of other lengths."""
    kps = kf.mvKeysUn
    vp = kf.get_map_point_matches()
    f = _bow_frame(kf, kps, vp)
    if f is None:
        return None
    n = len(f.desc)
    ur = kf.mvuRight
    if len(ur) != n:
        return None
    pts = [k.pt for k in kps]
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    if not (set(map(type, xs)) <= _F64_SET and set(map(type, ys)) <= _F64_SET):
        return None
    xy = np.empty((n, 2), np.float64)
    xy[:, 0], xy[:, 1] = xs, ys
    if not np.isfinite(xy).all():
        return None
    octs = [k.octave for k in kps]
    if not set(map(type, octs)) <= _INT_SET:
        return None
    octave = np.array(octs, np.int64)
    sf, sig = kf.mvScaleFactors, kf.mvLevelSigma2
    nl = min(len(sf), len(sig))
    if n and (int(octave.min()) < 0 or int(octave.max()) >= nl):  # a negative octave indexes from the end
        return None
    try:
        thr_ex = np.array([float(100 * sf[l]) for l in range(nl)], np.float64)
        thr_epi = np.array([float(3.84 * sig[l]) for l in range(nl)], np.float64)
    except (TypeError, ValueError):
        return None
    if not (np.isfinite(thr_ex).all() and np.isfinite(thr_epi).all()):
        return None
    t = _TriFrame()
    t.desc, t.angle, t.fv_node, t.fv_end, t.fv_idx = f.desc, f.angle, f.fv_node, f.fv_end, f.fv_idx
    t.xy, t.octave, t.thr_epi, t.thr_ex = xy, np.ascontiguousarray(octave, np.int32), thr_epi, thr_ex
    t.xy_f32 = bool(np.array_equal(xy.astype(np.float32).astype(np.float64), xy))
    free = np.fromiter(map(operator.not_, vp), bool, count=n)
    stereo = _u_right(kf) >= 0
    t.flags = (free * _lib.ORBFE_TRI_ELIGIBLE + stereo * _lib.ORBFE_TRI_STEREO).astype(np.uint8)
    return t


def _tri_epipole(ex, ey, f2):
    """(ex, ey) as doubles when the epipole gate of search_for_triangulation (ORBMatcher.py:650-653) is decided by
    k_tri_match's float64 arithmetic on the widened values, else None.  Doubles qualify as they are.  A float32
    epipole (float32 poses) makes the reference evaluate the gate in float32: with float32-valued positions every
    operation is then within 2^-24 relative of the double one, the whole left side within 2^-21, so the two agree
    unless a mono feature of frame 2 has its left side within thr * 2^-20 of its threshold, which is checked here."""
    vals = []
    for v in (ex, ey):
        if _is_f64(v):
            vals.append((float(v.item() if type(v) is np.ndarray else v), True))
        elif (type(v) is np.float32) or (type(v) is np.ndarray and v.dtype == np.float32 and v.size == 1):
            vals.append((float(v.item() if type(v) is np.ndarray else v), False))
        else:
            return None
    (x, xd), (y, yd) = vals
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    if not (xd and yd):
        if not f2.xy_f32:
            return None
        mono = (f2.flags & _lib.ORBFE_TRI_STEREO) == 0
        lhs = (x - f2.xy[mono, 0]) * (x - f2.xy[mono, 0]) + (y - f2.xy[mono, 1]) * (y - f2.xy[mono, 1])
        thr = f2.thr_ex[f2.octave[mono]]
        if bool((np.abs(lhs - thr) <= thr * 2.0 ** -20).any()):
            return None
    return x, y


def _search_arrays(fuse, kf_f64, kf_i32, off, xy, octave, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off, scale,
                   pt_f64, pt_desc, th, eps, u_right=None, inv_sigma2=None, blocked=None, sim3=None, fkf=None) -> dict:
    """fuse_search_arrays (fuse, with u_right and inv_sigma2), scw_search_arrays (not fuse, with blocked or None),
    sim3_search_arrays (not fuse, with sim3 = (srch_f64, srch_kf, srch_off, item_pt)) and fkf_search_arrays (not
    fuse, with blocked or None and fkf = (srch_kf, srch_off, item_pt)): the conversion, the length checks, the
    outputs and the call."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)
    kf_f64 = np.ascontiguousarray(kf_f64, np.float64).reshape(-1, _lib.ORBFE_FUSE_KF_F64)
    kf_i32 = np.ascontiguousarray(kf_i32, np.int32).reshape(-1, 3)
    pt_f64 = np.ascontiguousarray(pt_f64, np.float64).reshape(-1, _lib.ORBFE_FUSE_PT_F64)
    pt_desc = np.ascontiguousarray(pt_desc, np.uint8).reshape(-1, 32)
    off, cell_at, idx_at, lvl_off = (arr(a, np.int64) for a in (off, cell_at, idx_at, lvl_off))
    xy, u_right, scale, inv_sigma2 = (arr(a, np.float64) for a in (xy, u_right, scale, inv_sigma2))
    octave, cell_off, cell_idx = arr(octave, np.int32), arr(cell_off, np.int32), arr(cell_idx, np.int32)
    desc, blocked = arr(desc, np.uint8), arr(blocked, np.uint8)
    n_kf, n_pts = len(kf_f64), len(pt_f64)
    if len(kf_i32) != n_kf or len(pt_desc) != n_pts:
        raise ValueError("kf_i32 / pt_desc do not cover the keyframes / points")
    for a in (off, cell_at, idx_at, lvl_off):
        if a is None or len(a) != n_kf + 1:
            raise ValueError("an offset array does not have one entry per keyframe and one more")
    if n_kf:
        n, nc, ni, nl = int(off[-1]), int(cell_at[-1]), int(idx_at[-1]), int(lvl_off[-1])
        need = [(xy, 2 * n), (octave, n), (desc, 32 * n), (cell_off, nc), (cell_idx, ni), (scale, nl)]
        if fuse:
            need += [(u_right, n), (inv_sigma2, nl)]
        for a, size in need:
            if size > 0 and (a is None or a.size < size):
                raise ValueError("a per-keyframe array is shorter than its offsets say")
        if blocked is not None and blocked.size < n:
            raise ValueError("blocked does not have one byte per feature")
    grid = (ptr(cell_at), ptr(cell_off), ptr(idx_at), ptr(cell_idx), ptr(lvl_off), ptr(scale))
    if sim3 is not None or fkf is not None:
        if sim3 is not None:
            srch_f64 = np.ascontiguousarray(sim3[0], np.float64).reshape(-1, _lib.ORBFE_SIM3_F64)
            n_srch = len(srch_f64)
        else:
            sim3 = (None,) + tuple(fkf)
            n_srch = 0 if fkf[0] is None else int(np.size(fkf[0]))
        srch_kf, srch_off, item_pt = arr(sim3[1], np.int32), arr(sim3[2], np.int64), arr(sim3[3], np.int32)
        if srch_kf is None or srch_off is None or srch_kf.size != n_srch or srch_off.size != n_srch + 1:
            raise ValueError("srch_kf / srch_off do not cover the searches")
        n_items = int(srch_off[-1])
        if n_items > 0 and (item_pt is None or item_pt.size < n_items):
            raise ValueError("item_pt is shorter than srch_off says")
        n_items = max(n_items, 0)
        bi, bd, st = np.full(n_items, -1, np.int32), np.full(n_items, -1, np.int32), np.zeros(n_items, np.uint8)
        if fkf is not None:
            out = _lib.FkfOut(best_idx=bi.ctypes.data, best_dist=bd.ctypes.data, status=st.ctypes.data)
            call("orbfe_fkf_search", ptr(kf_f64), ptr(kf_i32), ptr(off), ptr(xy), ptr(octave), ptr(desc), ptr(blocked),
                 *grid, n_kf, ptr(pt_f64), ptr(pt_desc), n_pts, ptr(srch_kf), ptr(srch_off), n_srch, ptr(item_pt),
                 float(th), float(eps), C.byref(out))
            return dict(best_idx=bi, best_dist=bd, status=st)
        out = _lib.Sim3Out(best_idx=bi.ctypes.data, best_dist=bd.ctypes.data, status=st.ctypes.data)
        call("orbfe_sim3_search", ptr(kf_f64), ptr(kf_i32), ptr(off), ptr(xy), ptr(octave), ptr(desc), *grid, n_kf,
             ptr(pt_f64), ptr(pt_desc), n_pts, ptr(srch_f64), ptr(srch_kf), ptr(srch_off), n_srch, ptr(item_pt),
             float(th), float(eps), C.byref(out))
        return dict(best_idx=bi, best_dist=bd, status=st)
    bi = np.full((n_kf, n_pts), -1, np.int32)
    bd = np.full((n_kf, n_pts), -1, np.int32)
    st = np.zeros((n_kf, n_pts), np.uint8)
    out = (_lib.FuseOut if fuse else _lib.ScwOut)(best_idx=bi.ctypes.data, best_dist=bd.ctypes.data,
                                                  status=st.ctypes.data)
    if fuse:
        entry, kf = "orbfe_fuse_search", (ptr(xy), ptr(octave), ptr(u_right), ptr(desc)) + grid + (ptr(inv_sigma2),)
    else:
        entry, kf = "orbfe_scw_search", (ptr(xy), ptr(octave), ptr(desc), ptr(blocked)) + grid
    call(entry, ptr(kf_f64), ptr(kf_i32), ptr(off), *kf, n_kf, ptr(pt_f64), ptr(pt_desc), n_pts, float(th),
         float(eps), C.byref(out), n_pts)
    return dict(best_idx=bi, best_dist=bd, status=st)


def fuse_search_arrays(kf_f64, kf_i32, off, xy, octave, u_right, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                       scale, inv_sigma2, pt_f64, pt_desc, th, eps) -> dict:
    """orbfe_fuse_search (k_fuse_search, include/orbfe.h): the search half of ORBMatcher.fuse_pkf_mp
    (ORBMatcher.py:498-567) for every (keyframe, point) in one launch.  kf_f64 (K, 27) and kf_i32 (K, 3) hold the
    keyframes' scalars; keyframe k is features [off[k], off[k + 1]) of xy (x 2 f64) / octave (i32) / u_right (f64,
    negative: mono) / desc (x 32 u8), cell offsets [cell_at[k], cell_at[k + 1]) of cell_off, grid entries
    [idx_at[k], idx_at[k + 1]) of cell_idx and levels [lvl_off[k], lvl_off[k + 1]) of scale / inv_sigma2; pt_f64
    (P, 9) and pt_desc (P, 32) are the points.  Returns best_idx, best_dist (K, P) int32 (-1: no candidate) and
    status (K, P) uint8 (ORBFE_FUSE_MARGINAL)."""
    return _search_arrays(True, kf_f64, kf_i32, off, xy, octave, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                          scale, pt_f64, pt_desc, th, eps, u_right=u_right, inv_sigma2=inv_sigma2)


def scw_search_arrays(kf_f64, kf_i32, off, xy, octave, desc, blocked, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                      scale, pt_f64, pt_desc, th, eps) -> dict:
    """orbfe_scw_search (k_scw_search, include/orbfe.h): the search half of ORBMatcher.fuse_kf_scw_mp
    (ORBMatcher.py:409-468) and of search_by_projection_ckf_scw_mp (:863-916) for every (keyframe, point) in one
    launch.  The arrays are fuse_search_arrays' without u_right and inv_sigma2; the pose slots of kf_f64 hold what
    the Sim3 gives and its bf slot is not read.  blocked: None, or one byte per feature (concatenated at `off`),
    non-zero for a feature that is no candidate.  Returns best_idx, best_dist (K, P) int32 (-1: no candidate) and
    status (K, P) uint8 (ORBFE_FUSE_MARGINAL)."""
    return _search_arrays(False, kf_f64, kf_i32, off, xy, octave, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                          scale, pt_f64, pt_desc, th, eps, blocked=blocked)


def sim3_search_arrays(kf_f64, kf_i32, off, xy, octave, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off, scale,
                       pt_f64, pt_desc, srch_f64, srch_kf, srch_off, item_pt, th, eps) -> dict:
    """orbfe_sim3_search (k_sim3_search, include/orbfe.h): the search half of both directions of
    ORBMatcher.search_by_sim3 (ORBMatcher.py:742-789 and :791-838) for many keyframe pairs in one launch.  The
    keyframe arrays are scw_search_arrays' without blocked (each keyframe once; only the bounds, the inverse cell
    sizes and the log scale factor of kf_f64 are read), pt_f64 (P, 9) / pt_desc (P, 32) one shared point table (the
    normal is not read).  Search s has srch_f64[s] (28: fx fy cx cy, Rw, tw, sR, t), the target keyframe srch_kf[s]
    and the items [srch_off[s], srch_off[s + 1]) of item_pt, rows of the point table.  Returns best_idx, best_dist
    int32 (-1: no candidate) and status uint8 (ORBFE_FUSE_MARGINAL), flat over the items."""
    return _search_arrays(False, kf_f64, kf_i32, off, xy, octave, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                          scale, pt_f64, pt_desc, th, eps, sim3=(srch_f64, srch_kf, srch_off, item_pt))


def fkf_search_arrays(kf_f64, kf_i32, off, xy, octave, desc, blocked, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                      scale, pt_f64, pt_desc, srch_kf, srch_off, item_pt, th, eps) -> dict:
    """orbfe_fkf_search (k_fkf_search, include/orbfe.h): the search half of ORBMatcher.search_by_projection_f_kf_f
    (ORBMatcher.py:936-983, with Frame.get_features_in_area, Frame.py:373-416) for many (frame, map point list)
    searches in one launch.  The target arrays are scw_search_arrays' with a Frame in each block (the pose slots
    from mTcw and Ow = -Rcw^T tcw, the grid FRAME_GRID_COLS x FRAME_GRID_ROWS), blocked included: None, or one byte
    per feature, non-zero for a feature whose map point slot is taken.  pt_f64 (P, 9) / pt_desc (P, 32) are one
    shared point table (the normal is not read).  Search s has the target srch_kf[s] and the items
    [srch_off[s], srch_off[s + 1]) of item_pt, rows of the point table.  Returns best_idx, best_dist int32 (-1: no
    candidate) and status uint8 (ORBFE_FUSE_MARGINAL), flat over the items."""
    return _search_arrays(False, kf_f64, kf_i32, off, xy, octave, desc, cell_at, cell_off, idx_at, cell_idx, lvl_off,
                          scale, pt_f64, pt_desc, th, eps, blocked=blocked, fkf=(srch_kf, srch_off, item_pt))


LOCAL_OUTPUTS = ("in_view", "level", "best_idx", "best_dist", "second_idx", "second_dist", "status")


def local_search_arrays(kf_f64, kf_i32, off, xy, octave, u_right, desc, blocked, cell_at, cell_off, idx_at, cell_idx,
                        lvl_off, scale, pt_f64, pt_desc, srch_limit, srch_kf, srch_off, item_pt, th, th_on,
                        eps) -> dict:
    """orbfe_local_search (k_local_search, include/orbfe.h): Frame.is_in_frustum (Frame.py:328-371) and the search
    half of ORBMatcher.search_by_projection_f_p (ORBMatcher.py:215-283) for many (frame, local map) searches in one
    launch.  The target arrays are fkf_search_arrays' with u_right (<= 0: no stereo gate) and the bf slot of kf_f64
    read; pt_f64 (P, 9) / pt_desc (P, 32) are one shared point table, the normal read.  Search s has the viewing
    cosine's limit srch_limit[s], the target srch_kf[s] and the items [srch_off[s], srch_off[s + 1]) of item_pt.  th
    multiplies the radius only where th_on is true (the caller's th != 1.0).  Returns, flat over the items: in_view
    uint8, level int32 (-1: not in view), best_idx, best_dist, second_idx, second_dist int32 (-1: none) and status
    uint8 (ORBFE_FUSE_MARGINAL)."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)
    kf_f64 = np.ascontiguousarray(kf_f64, np.float64).reshape(-1, _lib.ORBFE_FUSE_KF_F64)
    kf_i32 = np.ascontiguousarray(kf_i32, np.int32).reshape(-1, 3)
    pt_f64 = np.ascontiguousarray(pt_f64, np.float64).reshape(-1, _lib.ORBFE_FUSE_PT_F64)
    pt_desc = np.ascontiguousarray(pt_desc, np.uint8).reshape(-1, 32)
    off, cell_at, idx_at, lvl_off = (arr(a, np.int64) for a in (off, cell_at, idx_at, lvl_off))
    xy, u_right, scale, srch_limit = (arr(a, np.float64) for a in (xy, u_right, scale, srch_limit))
    octave, cell_off, cell_idx = arr(octave, np.int32), arr(cell_off, np.int32), arr(cell_idx, np.int32)
    desc, blocked = arr(desc, np.uint8), arr(blocked, np.uint8)
    n_kf, n_pts = len(kf_f64), len(pt_f64)
    if len(kf_i32) != n_kf or len(pt_desc) != n_pts:
        raise ValueError("kf_i32 / pt_desc do not cover the keyframes / points")
    for a in (off, cell_at, idx_at, lvl_off):
        if a is None or len(a) != n_kf + 1:
            raise ValueError("an offset array does not have one entry per keyframe and one more")
    if n_kf:
        n, nc, ni, nl = int(off[-1]), int(cell_at[-1]), int(idx_at[-1]), int(lvl_off[-1])
        for a, size in ((xy, 2 * n), (octave, n), (u_right, n), (desc, 32 * n), (cell_off, nc), (cell_idx, ni),
                        (scale, nl)):
            if size > 0 and (a is None or a.size < size):
                raise ValueError("a per-keyframe array is shorter than its offsets say")
        if blocked is not None and blocked.size < n:
            raise ValueError("blocked does not have one byte per feature")
    n_srch = 0 if srch_kf is None else int(np.size(srch_kf))
    srch_kf, srch_off, item_pt = arr(srch_kf, np.int32), arr(srch_off, np.int64), arr(item_pt, np.int32)
    if srch_kf is None or srch_off is None or srch_off.size != n_srch + 1 or (
            n_srch and (srch_limit is None or srch_limit.size != n_srch)):
        raise ValueError("srch_limit / srch_kf / srch_off do not cover the searches")
    n_items = int(srch_off[-1])
    if n_items > 0 and (item_pt is None or item_pt.size < n_items):
        raise ValueError("item_pt is shorter than srch_off says")
    n_items = max(n_items, 0)
    res = {k: (np.zeros(n_items, np.uint8) if k in ("in_view", "status") else np.full(n_items, -1, np.int32))
           for k in LOCAL_OUTPUTS}
    out = _lib.LocalOut(**{k: v.ctypes.data for k, v in res.items()})
    call("orbfe_local_search", ptr(kf_f64), ptr(kf_i32), ptr(off), ptr(xy), ptr(octave), ptr(u_right), ptr(desc),
         ptr(blocked), ptr(cell_at), ptr(cell_off), ptr(idx_at), ptr(cell_idx), ptr(lvl_off), ptr(scale), n_kf,
         ptr(pt_f64), ptr(pt_desc), n_pts, ptr(srch_limit), ptr(srch_kf), ptr(srch_off), n_srch, ptr(item_pt),
         float(th), 1 if th_on else 0, float(eps), C.byref(out))
    return res


def local_search_last_ms() -> float:
    """Kernel time of the last local_search_arrays call (ms, HIP events)."""
    ms = C.c_float(0.0)
    call("orbfe_local_search_last_ms", C.byref(ms))
    return float(ms.value)


FF_OUTPUTS = ("best_idx", "best_dist", "status")


def ff_search_arrays(kf_f64, kf_i32, off, xy, octave, u_right, desc, blocked, cell_at, cell_off, idx_at, cell_idx,
                     lvl_off, scale, pt_f64, pt_desc, srch_th, srch_mode, srch_kf, srch_off, item_pt, item_level,
                     eps) -> dict:
    """orbfe_ff_search (k_ff_search, include/orbfe.h): the search half of ORBMatcher.search_by_projection_f_f
    (ORBMatcher.py:291-393, with Frame.get_features_in_area, Frame.py:373-416) for many (current frame, last frame)
    pairs in one launch.  The target arrays are local_search_arrays' (the current frames), u_right and blocked
    included; pt_f64 (P, 9) / pt_desc (P, 32) are one shared point table of which only the position is read.  Search
    s has its th srch_th[s], its octave mode srch_mode[s] (0: [level - 1, level + 1], 1 forward: [level, inf), 2
    backward: [0, level]), the target srch_kf[s] and the items [srch_off[s], srch_off[s + 1]) of item_pt / item_level
    (the point's row and the octave of the last frame's keypoint).  Returns best_idx, best_dist int32 (-1: no
    candidate) and status uint8 (ORBFE_FUSE_MARGINAL), flat over the items."""
    def arr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)
    kf_f64 = np.ascontiguousarray(kf_f64, np.float64).reshape(-1, _lib.ORBFE_FUSE_KF_F64)
    kf_i32 = np.ascontiguousarray(kf_i32, np.int32).reshape(-1, 3)
    pt_f64 = np.ascontiguousarray(pt_f64, np.float64).reshape(-1, _lib.ORBFE_FUSE_PT_F64)
    pt_desc = np.ascontiguousarray(pt_desc, np.uint8).reshape(-1, 32)
    off, cell_at, idx_at, lvl_off = (arr(a, np.int64) for a in (off, cell_at, idx_at, lvl_off))
    xy, u_right, scale, srch_th = (arr(a, np.float64) for a in (xy, u_right, scale, srch_th))
    octave, cell_off, cell_idx = arr(octave, np.int32), arr(cell_off, np.int32), arr(cell_idx, np.int32)
    desc, blocked = arr(desc, np.uint8), arr(blocked, np.uint8)
    n_kf, n_pts = len(kf_f64), len(pt_f64)
    if len(kf_i32) != n_kf or len(pt_desc) != n_pts:
        raise ValueError("kf_i32 / pt_desc do not cover the keyframes / points")
    for a in (off, cell_at, idx_at, lvl_off):
        if a is None or len(a) != n_kf + 1:
            raise ValueError("an offset array does not have one entry per keyframe and one more")
    if n_kf:
        n, nc, ni, nl = int(off[-1]), int(cell_at[-1]), int(idx_at[-1]), int(lvl_off[-1])
        for a, size in ((xy, 2 * n), (octave, n), (u_right, n), (desc, 32 * n), (cell_off, nc), (cell_idx, ni),
                        (scale, nl)):
            if size > 0 and (a is None or a.size < size):
                raise ValueError("a per-keyframe array is shorter than its offsets say")
        if blocked is not None and blocked.size < n:
            raise ValueError("blocked does not have one byte per feature")
    n_srch = 0 if srch_kf is None else int(np.size(srch_kf))
    srch_kf, srch_off, srch_mode = arr(srch_kf, np.int32), arr(srch_off, np.int64), arr(srch_mode, np.int32)
    item_pt, item_level = arr(item_pt, np.int32), arr(item_level, np.int32)
    if srch_kf is None or srch_off is None or srch_off.size != n_srch + 1 or (
            n_srch and (srch_th is None or srch_th.size != n_srch or srch_mode is None or srch_mode.size != n_srch)):
        raise ValueError("srch_th / srch_mode / srch_kf / srch_off do not cover the searches")
    n_items = int(srch_off[-1])
    if n_items > 0 and (item_pt is None or item_pt.size < n_items or item_level is None or item_level.size < n_items):
        raise ValueError("item_pt / item_level are shorter than srch_off says")
    n_items = max(n_items, 0)
    res = dict(best_idx=np.full(n_items, -1, np.int32), best_dist=np.full(n_items, -1, np.int32),
               status=np.zeros(n_items, np.uint8))
    out = _lib.FfOut(**{k: v.ctypes.data for k, v in res.items()})
    call("orbfe_ff_search", ptr(kf_f64), ptr(kf_i32), ptr(off), ptr(xy), ptr(octave), ptr(u_right), ptr(desc),
         ptr(blocked), ptr(cell_at), ptr(cell_off), ptr(idx_at), ptr(cell_idx), ptr(lvl_off), ptr(scale), n_kf,
         ptr(pt_f64), ptr(pt_desc), n_pts, ptr(srch_th), ptr(srch_mode), ptr(srch_kf), ptr(srch_off), n_srch,
         ptr(item_pt), ptr(item_level), float(eps), C.byref(out))
    return res


def ff_search_last_ms() -> float:
    """Kernel time of the last ff_search_arrays call (ms, HIP events)."""
    ms = C.c_float(0.0)
    call("orbfe_ff_search_last_ms", C.byref(ms))
    return float(ms.value)


# eps of orbfe_fuse_search: the unit of rounding of the reference's arithmetic, with a factor 2 in hand for
# float32 (2^-24 is its unit roundoff) and the 2^-48 class of k_tri_match for float64
FUSE_EPS_F32 = 2.0 ** -23
FUSE_EPS_F64 = 2.0 ** -48
_POSE_DT = (np.dtype(np.float32), np.dtype(np.float64))
_F32_DT = np.dtype(np.float32)
_TH_SET = frozenset((int, float, np.float64))
_DIST_SET = frozenset((float, np.float64, np.float32))
_fuse_cache = weakref.WeakKeyDictionary()


class _FuseFrame:
    __slots__ = ("f64", "i32", "xy", "octave", "u_right", "desc", "cell_off", "cell_idx", "scale", "inv_sigma2", "f32",
                 "pose")


def _pose_part(a, shape):
    """a as a flat list of doubles (widened exactly) and whether it was float32; None unless it is a finite
    float32 / float64 array of that shape."""
    if not (type(a) is np.ndarray and a.shape == shape and a.dtype in _POSE_DT and bool(np.isfinite(a).all())):
        return None
    return a.astype(np.float64).reshape(-1).tolist(), a.dtype == _F32_DT


def _fuse_static(kf, dims=None):
    """(xy, octave, desc, cell_off, cell_idx) of a keyframe, cached while mvKeysUn, mDescriptors and mGrid are the
    same objects; None for what the arrays cannot express.  dims: the grid's (columns, rows) where they are not
    mnGridCols / mnGridRows (a Frame's FRAME_GRID_COLS / FRAME_GRID_ROWS)."""
    kps, descs, grid = kf.mvKeysUn, kf.mDescriptors, kf.mGrid
    try:
        ent = _fuse_cache.get(kf)
    except TypeError:
        ent = None
    if ent is not None and ent[0] is kps and ent[1] is descs and ent[2] is grid and ent[3] == len(kps):
        return ent[4]
    n = len(kps)
    cols, rows = dims if dims is not None else (kf.mnGridCols, kf.mnGridRows)
    if not (type(cols) in _INT_SET and type(rows) in _INT_SET and 0 < cols <= 4096 and 0 < rows <= 4096):
        return None
    if n > _lib.ORBFE_BOW_MAX_FRAME:
        return None
    if not (type(descs) is np.ndarray and descs.dtype == _U8_DT and descs.shape == (n, 32)):
        return None
    pts = [k.pt for k in kps]
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    octs = [k.octave for k in kps]
    if not (set(map(type, xs)) <= _F64_SET and set(map(type, ys)) <= _F64_SET and set(map(type, octs)) <= _INT_SET):
        return None
    xy = np.empty((n, 2), np.float64)
    xy[:, 0], xy[:, 1] = xs, ys
    if not np.isfinite(xy).all():
        return None
    if len(grid) != cols or any(len(col) != rows for col in grid):
        return None
    sizes = np.fromiter((len(cell) for col in grid for cell in col), np.int64, count=cols * rows)
    total = int(sizes.sum())
    if total > _lib.ORBFE_BOW_MAX_FRAME:
        return None
    flat = [g for col in grid for cell in col for g in cell]
    if not set(map(type, flat)) <= _INT_SET:
        return None
    cell_idx = np.array(flat, np.int64).reshape(-1)
    if total and (int(cell_idx.min()) < 0 or int(cell_idx.max()) >= n):  # a negative index counts from the end
        return None
    cell_off = np.zeros(cols * rows + 1, np.int32)
    np.cumsum(sizes, out=cell_off[1:])
    val = (xy, np.array(octs, np.int64).astype(np.int32).reshape(-1), np.ascontiguousarray(descs),
           cell_off, cell_idx.astype(np.int32))
    try:
        _fuse_cache[kf] = (kps, descs, grid, n, val)
    except TypeError:
        pass
    return val


def _fuse_frame(kf):
    """Array form of a keyframe for k_fuse_search: the scalars of include/orbfe.h's layout (the pose read anew on
    every call, as its getters return it), the undistorted positions, octaves, right coordinates, descriptors,
    level tables and the grid as CSR in the reference's visiting order.  None when the arrays cannot express the
    keyframe (the caller then takes fuse_pkf_mp): intrinsics or grid parameters that are not plain doubles, a pose
    that is not a finite float32 / float64 array of its shape, more features or grid entries than
    ORBFE_BOW_MAX_FRAME, a keypoint field, mvuRight entry or level table entry of another type, an octave outside
    the level tables."""
    sc = (kf.fx, kf.fy, kf.cx, kf.cy, kf.mbf)
    gr = (kf.mnMinX, kf.mnMaxX, kf.mnMinY, kf.mnMaxY, kf.mfGridElementWidthInv, kf.mfGridElementHeightInv,
          kf.mfLogScaleFactor)
    if not (set(map(type, sc)) <= _F64_SET and set(map(type, gr)) <= _F64_SET):
        return None
    levels = kf.mnScaleLevels
    if type(levels) not in _INT_SET or levels <= 0:
        return None
    R, t, O = _pose_part(kf.get_rotation(), (3, 3)), _pose_part(kf.get_translation(), (3, 1)), _pose_part(
        kf.get_camera_center(), (3, 1))
    if R is None or t is None or O is None:
        return None
    st = _fuse_static(kf)
    if st is None:
        return None
    xy, octave, desc, cell_off, cell_idx = st
    n = len(xy)
    sf, is2 = kf.mvScaleFactors, kf.mvInvLevelSigma2
    if len(sf) < levels or len(is2) < levels:
        return None
    sf, is2 = list(sf[:levels]), list(is2[:levels])
    if not (set(map(type, sf)) <= _F64_SET and set(map(type, is2)) <= _F64_SET):
        return None
    ur = kf.mvuRight
    if len(ur) != n or not set(map(type, ur)) <= _UR_SET:
        return None
    u_right = _u_right(kf)
    f64 = np.array(list(sc) + R[0] + t[0] + O[0] + list(gr), np.float64)
    scale, inv_sigma2 = np.array(sf, np.float64), np.array(is2, np.float64)
    if not (np.isfinite(f64).all() and np.isfinite(scale).all() and np.isfinite(inv_sigma2).all()
            and np.isfinite(u_right).all()):
        return None
    if n and (int(octave.min()) < 0 or int(octave.max()) >= levels):
        return None
    f = _FuseFrame()
    f.f64, f.i32 = f64, np.array([kf.mnGridCols, kf.mnGridRows, levels], np.int32)
    f.xy, f.octave, f.u_right, f.desc, f.cell_off, f.cell_idx = xy, octave, u_right, desc, cell_off, cell_idx
    f.scale, f.inv_sigma2 = scale, inv_sigma2
    f.f32 = R[1] or t[1] or O[1]
    return f


def _fkf_frame(F, int_bounds=False):
    """Array form of a Frame for k_fkf_search, with the surface search_by_projection_f_kf_f and
    Frame.get_features_in_area read (Frame.py): the _FuseFrame of _fuse_frame without right coordinates and inverse
    sigma squares, the grid FRAME_GRID_COLS x FRAME_GRID_ROWS, the bf slot 0.0 (not read), the pose slots from mTcw
    and Ow = -Rcw^T tcw by the reference's expression, kept in f.pose as (Rcw, tcw, Ow).  None when the arrays cannot
    express the frame (the caller then takes the host body): an attribute of that surface is missing, intrinsics or
    grid parameters are not plain doubles, mTcw is not a finite 4 x 4 float32 / float64 array or the centre it
    gives is not finite, and what _fuse_static and _fuse_frame refuse in a keyframe's features, grid and scale
    table.  int_bounds (k_local_search): an image bound may also be a plain int below 2^53, which every comparison and
    difference the reference makes with it takes at its exact value (Tracking passes the image's width and height
    as mnMaxX and mnMaxY where there is no distortion)."""
    try:
        sc = (F.fx, F.fy, F.cx, F.cy)
        gr = (F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY, F.mfGridElementWidthInv, F.mfGridElementHeightInv,
              F.mfLogScaleFactor)
        dims, levels, sf, T = (F.FRAME_GRID_COLS, F.FRAME_GRID_ROWS), F.mnScaleLevels, F.mvScaleFactors, F.mTcw
    except AttributeError:
        return None
    if int_bounds and all(type(b) is not int or abs(b) < 2 ** 53 for b in gr[:4]):
        gr = tuple(float(b) if type(b) is int else b for b in gr[:4]) + gr[4:]
    if not (set(map(type, sc)) <= _F64_SET and set(map(type, gr)) <= _F64_SET):
        return None
    if type(levels) not in _INT_SET or levels <= 0:
        return None
    if not (type(T) is np.ndarray and T.shape == (4, 4) and T.dtype in _POSE_DT and bool(np.isfinite(T).all())):
        return None
    Rcw, tcw = T[:3, :3], T[:3, 3:4]
    with np.errstate(all="ignore"):
        Ow = -np.dot(Rcw.T, tcw)
    R, t, O = _pose_part(Rcw, (3, 3)), _pose_part(tcw, (3, 1)), _pose_part(Ow, (3, 1))
    if R is None or t is None or O is None:
        return None
    st = _fuse_static(F, dims)
    if st is None:
        return None
    xy, octave, desc, cell_off, cell_idx = st
    if len(cell_off) != dims[0] * dims[1] + 1:  # cached for the same mGrid under another FRAME_GRID_COLS / ROWS
        return None
    if len(sf) < levels:
        return None
    sf = list(sf[:levels])
    if not set(map(type, sf)) <= _F64_SET:
        return None
    f64, scale = np.array(list(sc) + [0.0] + R[0] + t[0] + O[0] + list(gr), np.float64), np.array(sf, np.float64)
    if not (np.isfinite(f64).all() and np.isfinite(scale).all()):
        return None
    if len(xy) and (int(octave.min()) < 0 or int(octave.max()) >= levels):
        return None
    f = _FuseFrame()
    f.f64, f.i32 = f64, np.array([dims[0], dims[1], levels], np.int32)
    f.xy, f.octave, f.desc, f.cell_off, f.cell_idx, f.scale = xy, octave, desc, cell_off, cell_idx, scale
    f.f32, f.pose = T.dtype == _F32_DT, (Rcw, tcw, Ow)
    return f


def _local_frame(F):
    """Array form of a Frame for k_local_search, with the surface Frame.is_in_frustum and search_by_projection_f_p
    read: _fkf_frame's (an image bound may be a plain int), with the bf slot from mbf, the pose slots from mRcw, mtcw and mOw (what is_in_frustum
    projects with; set_pose derives them from mTcw) and the right coordinates of mvuRight.  None when _fkf_frame
    refuses the frame, when one of those attributes is missing, when mbf is not a plain finite double, when a pose part
    is not a finite float32 / float64 array of its shape, or when mvuRight does not hold one int / float / np.float32 /
    np.float64 per feature."""
    f = _fkf_frame(F, int_bounds=True)
    if f is None:
        return None
    try:
        bf, parts, ur = F.mbf, (F.mRcw, F.mtcw, F.mOw), F.mvuRight
    except AttributeError:
        return None
    if type(bf) not in _F64_SET or not np.isfinite(bf):
        return None
    R, t, O = _pose_part(parts[0], (3, 3)), _pose_part(parts[1], (3, 1)), _pose_part(parts[2], (3, 1))
    if R is None or t is None or O is None:
        return None
    if len(ur) != len(f.xy) or not set(map(type, ur)) <= _UR_SET:
        return None
    u_right = _u_right(F)
    if not np.isfinite(u_right).all():
        return None
    f.f64 = f.f64.copy()
    f.f64[4] = bf
    f.f64[5:20] = R[0] + t[0] + O[0]
    f.u_right = u_right
    f.f32 = R[1] or t[1] or O[1]
    return f


def _ff_frame(F):
    """Array form of a current Frame for k_ff_search, with the surface search_by_projection_f_f and
    Frame.get_features_in_area read: _fkf_frame's (the pose slots from mTcw, which the search projects with), with the
    bf slot from mbf and the right coordinates of mvuRight as _local_frame takes them.  None when _fkf_frame refuses
    the frame, when mbf or mvuRight is missing, when mbf is not a plain finite double, or when mvuRight does not hold
    one finite int / float / np.float32 / np.float64 per feature.  An image bound may be a plain int, as in
    _local_frame."""
    f = _fkf_frame(F, int_bounds=True)
    if f is None:
        return None
    try:
        bf, ur = F.mbf, F.mvuRight
    except AttributeError:
        return None
    if type(bf) not in _F64_SET or not np.isfinite(bf):
        return None
    if len(ur) != len(f.xy) or not set(map(type, ur)) <= _UR_SET:
        return None
    u_right = _u_right(F)
    if not np.isfinite(u_right).all():
        return None
    f.f64 = f.f64.copy()
    f.f64[4] = bf
    f.u_right = u_right
    return f


def _fuse_point(pMP, normal=True, f32_dist=False):
    """(9 doubles, descriptor row, any float32) of a map point for k_fuse_search, or None when the arrays cannot
    express it: a position or normal that is not a finite (3, 1) float32 / float64 array, distances that are not
    plain doubles, a descriptor that is not 32 bytes of uint8.  normal False (k_fkf_search, whose reference never
    asks for it): get_normal is not called and the slots hold zeros.  f32_dist (k_local_search): a distance may also
    be an np.float32, which a map point made from a float32 pose holds; it is widened exactly, as the reference's
    comparison with a float64 distance widens it (against a float32 distance the caller's eps is float32's)."""
    p = _pose_part(pMP.get_world_pos(), (3, 1))
    nrm = _pose_part(pMP.get_normal(), (3, 1)) if normal else ([0.0, 0.0, 0.0], False)
    if p is None or nrm is None:
        return None
    d3 = (pMP.get_min_distance_invariance(), pMP.get_max_distance_invariance(), pMP.mfMaxDistance)
    if not set(map(type, d3)) <= (_DIST_SET if f32_dist else _F64_SET) or not all(map(np.isfinite, d3)):
        return None
    d3 = tuple(map(float, d3))
    d = pMP.get_descriptor()
    if not (type(d) is np.ndarray and d.dtype == _U8_DT and d.size == 32):
        return None
    return p[0] + nrm[0] + list(d3), d.reshape(32), p[1] or nrm[1]


class ORBMatcher:
    def __init__(self, nnratio=1, checkOri=True):
        self.mfNNratio = nnratio
        self.mbCheckOrientation = checkOri

    # ORBMatcher.py:12-14 (one pair, on the host in liborbfe; use descriptor_distances / hamming_* for batches)
    def descriptor_distance(self, a, b):
        return descriptor_distance(a, b)

    def descriptor_distances(self, A, B):
        return hamming_matrix(A, B)

    def compute_three_maxima(self, histo, histo_length):
        histo_counts = [len(h) for h in histo]
        return np.argsort(histo_counts)[::-1][:3]

    def radius_by_viewing_cos(self, view_cos):
        return 2.5 if view_cos > 0.998 else 4.0

    @staticmethod
    def _csr(qd, train, off, idx):
        """The one device call of a search: distances of CSR (query, candidate) pairs."""
        return hamming_csr(qd, train, off, idx)

    @classmethod
    def _batched(cls, queries, train):
        """queries: list of (descriptor, candidate list) -> list of distance arrays."""
        off = np.zeros(len(queries) + 1, np.int32)
        for i, (_, c) in enumerate(queries):
            off[i + 1] = off[i] + len(c)
        if not queries or off[-1] == 0:
            return [np.zeros(0, np.int32) for _ in queries]
        qd = np.stack([np.asarray(d, np.uint8).reshape(32) for d, _ in queries])
        idx = np.concatenate([np.asarray(c, np.int32) for _, c in queries])
        dist = cls._csr(qd, train, off, idx)
        return [dist[off[i]:off[i + 1]] for i in range(len(queries))]

    def _nonempty(self, off, idx, pmps, train):
        """Restrict a CSR candidate set to its non-empty queries and get their distances: (rows, off, dist),
        rows = indices of the non-empty queries (the reference fetches a descriptor only for those)."""
        cnt = np.diff(off)
        rows = np.flatnonzero(cnt)
        off2 = np.zeros(len(rows) + 1, np.int32)
        np.cumsum(cnt[rows], out=off2[1:])
        if len(rows) == 0:
            return rows, off2, np.zeros(0, np.int32)
        qd = _descriptor_rows(list(map(_DESCRIPTOR, map(pmps.__getitem__, rows.tolist()))))
        return rows, off2, np.ascontiguousarray(self._csr(qd, train, off2, idx), np.int32)

    # ORBMatcher.py:215-283
    def _f_p_inputs(self, vp_map_points, th, b_factor):
        """The searched map points of search_by_projection_f_p (tracked in view, then not bad: the reference's
        two `continue`s in its order), their predicted levels and radii, with the per-point attribute reads
        and calls as map() over C-level getters.  The radius is ORBMatcher's own radius_by_viewing_cos
        evaluated over an array of doubles (`vc > 0.998` in double, then `r *= th`), or point by point when a
        view cosine is not a double (a float32 one compares in float32); None (run the reference loop) when
        the method is overridden or th is not a Python number."""
        if type(self).radius_by_viewing_cos is not ORBMatcher.radius_by_viewing_cos:
            return None
        if b_factor and type(th) not in (int, float):
            return None
        cand = list(compress(vp_map_points, map(_IN_VIEW, vp_map_points)))
        pmps = list(compress(cand, map(operator.not_, map(_IS_BAD, cand))))
        cos = list(map(_VIEW_COS, pmps))
        vc = _f64_array(cos)
        if vc is None:
            # not all doubles: the reference's per-point radius on the points already selected (no
            # second mbTrackInView / is_bad() pass through the reference loop)
            radius = self.radius_by_viewing_cos
            rads = []
            for c in cos:
                r = radius(c)
                if b_factor:
                    r *= th
                rads.append(r)
            return pmps, list(map(_TRACK_LEVEL, pmps)), rads
        r = np.where(vc > 0.998, 2.5, 4.0)
        if b_factor:
            r = r * th
        return pmps, list(map(_TRACK_LEVEL, pmps)), r.tolist()

    def search_by_projection_f_p(self, frame, vp_map_points, th):
        n_matches = 0
        b_factor = th != 1.0
        radius = self.radius_by_viewing_cos
        pre = self._f_p_inputs(vp_map_points, th, b_factor) if isinstance(vp_map_points, (list, tuple)) else None
        if pre is not None:
            pmps, lvls, rads = pre
        else:
            pmps, lvls, rads = [], [], []
            for pMP in vp_map_points:
                if not pMP.mbTrackInView:
                    continue
                if pMP.is_bad():
                    continue
                r = radius(pMP.mTrackViewCos)
                if b_factor:
                    r *= th
                pmps.append(pMP)
                lvls.append(pMP.mnTrackScaleLevel)
                rads.append(r)
        done = self._f_p_native(frame, pmps, lvls, rads)
        if done is not None:
            return done
        sf = frame.mvScaleFactors
        pend = list(zip(pmps, lvls, rads))
        queries = [(p.mTrackProjX, p.mTrackProjY, r * sf[lv], lv - 1, lv) for p, lv, r in pend]
        work = [(pMP, lvl, r, v_indices, pMP.get_descriptor())
                for (pMP, lvl, r), v_indices in zip(pend, features_in_areas(frame, queries)) if v_indices]
        dists = self._batched([(w[4], w[3]) for w in work], frame.mDescriptors)
        for (pMP, n_predicted_level, r, v_indices, _), dq in zip(work, dists):
            best_dist = 256
            best_level = -1
            best_dist2 = 256
            best_level2 = -1
            best_idx = -1
            for idx, dist in zip(v_indices, dq.tolist()):
                if frame.mvpMapPoints[idx]:
                    if frame.mvpMapPoints[idx].observations() > 0:
                        continue
                if frame.mvuRight[idx] > 0:
                    er = abs(pMP.mTrackProjXR - frame.mvuRight[idx])
                    if er > r * frame.mvScaleFactors[n_predicted_level]:
                        continue
                if dist < best_dist:
                    best_dist2 = best_dist
                    best_dist = dist
                    best_level2 = best_level
                    best_level = frame.mvKeysUn[idx].octave
                    best_idx = idx
                elif dist < best_dist2:
                    best_level2 = frame.mvKeysUn[idx].octave
                    best_dist2 = dist
            if best_dist <= TH_HIGH:
                if best_level == best_level2 and best_dist > self.mfNNratio * best_dist2:
                    continue
                frame.mvpMapPoints[best_idx] = pMP
                n_matches += 1
        return n_matches

    # ORBMatcher.py:291-393
    def search_by_projection_f_f(self, current_frame, last_frame, th):
        n_matches = 0
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        factor = 1.0 / HISTO_LENGTH
        Rcw = current_frame.mTcw[:3, :3]
        tcw = current_frame.mTcw[:3, 3:4]
        twc = -Rcw.T @ tcw
        Rlw = last_frame.mTcw[:3, :3]
        tlw = last_frame.mTcw[:3, 3:4]
        tlc = Rlw @ twc + tlw
        b_forward = tlc[2] > current_frame.mb
        b_backward = -tlc[2] > current_frame.mb
        # projection of every usable map point of the last frame (one stacked matmul: the same per-point
        # BLAS product as `Rcw @ x3Dw`, element-wise arithmetic in the reference's order and dtypes)
        lmps, lout, n_last = last_frame.mvpMapPoints, last_frame.mvbOutlier, last_frame.N
        if len(lmps) >= n_last and len(lout) >= n_last:
            # [i for i in range(n_last) if lmps[i] and not lout[i]] with C-level iteration (bool(m): the
            # truth test `if m` makes; `not lout[i]` only where lmps[i] is true, as the reference's `and`)
            live = list(compress(range(n_last), map(bool, lmps)))
            cand = list(compress(live, map(operator.not_, map(lout.__getitem__, live))))
        else:  # the reference's indexing (and its IndexError)
            cand = [i for i in range(n_last) if lmps[i] and not lout[i]]
        pos = list(map(_WORLD_POS, map(lmps.__getitem__, cand)))
        proj = []
        if (pos and set(map(type, pos)) == _NDARRAY_SET and set(map(_SHAPE, pos)) == {(3, 1)}
                and len(set(map(_DTYPE, pos))) == 1):
            x3Dc = Rcw @ np.concatenate(pos).reshape(len(pos), 3, 1) + tcw  # np.stack(pos), 3x faster
            zc = x3Dc[:, 2, 0]
            invzc = 1.0 / zc
            u = current_frame.fx * x3Dc[:, 0, 0] * invzc + current_frame.cx
            v = current_frame.fy * x3Dc[:, 1, 0] * invzc + current_frame.cy
            keep = ~((invzc < 0) | (u < current_frame.mnMinX) | (u > current_frame.mnMaxX) |
                     (v < current_frame.mnMinY) | (v > current_frame.mnMaxY))
            sel = np.flatnonzero(keep)
            done = self._f_f_native(current_frame, last_frame, th, b_forward, b_backward, cand, sel, u, v, invzc)
            if done is not None:
                return done
            proj = [(cand[k], u[k], v[k], invzc[k]) for k in sel.tolist()]
        else:
            for i, x3Dw in zip(cand, pos):
                x3Dc = Rcw @ x3Dw + tcw
                xc, yc, zc = x3Dc[0][0], x3Dc[1][0], x3Dc[2][0]
                invzc = 1.0 / zc
                if invzc < 0:
                    continue
                u = current_frame.fx * xc * invzc + current_frame.cx
                v = current_frame.fy * yc * invzc + current_frame.cy
                if u < current_frame.mnMinX or u > current_frame.mnMaxX:
                    continue
                if v < current_frame.mnMinY or v > current_frame.mnMaxY:
                    continue
                proj.append((i, u, v, invzc))
        queries, pend = [], []
        for i, u, v, invzc in proj:
            n_last_octave = last_frame.mvKeys[i].octave
            radius = th * current_frame.mvScaleFactors[n_last_octave]
            if b_forward:
                queries.append((u, v, radius, n_last_octave, -1))
            elif b_backward:
                queries.append((u, v, radius, 0, n_last_octave))
            else:
                queries.append((u, v, radius, n_last_octave - 1, n_last_octave + 1))
            pend.append((i, u, invzc, radius))
        work = []
        for (i, u, invzc, radius), v_indices2 in zip(pend, features_in_areas(current_frame, queries)):
            if not v_indices2:
                continue
            pMP = last_frame.mvpMapPoints[i]
            work.append((i, pMP, u, invzc, radius, v_indices2, pMP.get_descriptor()))
        dists = self._batched([(w[6], w[5]) for w in work], current_frame.mDescriptors)
        for (i, pMP, u, invzc, radius, v_indices2, _), dq in zip(work, dists):
            best_dist = 256
            best_idx2 = -1
            for i2, dist in zip(v_indices2, dq.tolist()):
                if current_frame.mvpMapPoints[i2]:
                    if current_frame.mvpMapPoints[i2].observations() > 0:
                        continue
                if current_frame.mvuRight[i2] > 0:
                    ur = u - current_frame.mbf * invzc
                    er = abs(ur - current_frame.mvuRight[i2])
                    if er > radius:
                        continue
                if dist < best_dist:
                    best_dist = dist
                    best_idx2 = i2
            if best_dist <= TH_HIGH:
                current_frame.mvpMapPoints[best_idx2] = pMP
                n_matches += 1
                if self.mbCheckOrientation:
                    rot = last_frame.mvKeysUn[i].angle - current_frame.mvKeysUn[best_idx2].angle
                    if rot < 0.0:
                        rot += 360.0
                    bin_idx = round(rot * factor)
                    if bin_idx == HISTO_LENGTH:
                        bin_idx = 0
                    assert 0 <= bin_idx < HISTO_LENGTH
                    rot_hist[bin_idx].append(best_idx2)
        if self.mbCheckOrientation:
            ind1, ind2, ind3 = self.compute_three_maxima(rot_hist, HISTO_LENGTH)
            for i in range(HISTO_LENGTH):
                if i not in (ind1, ind2, ind3):
                    for idx in rot_hist[i]:
                        current_frame.mvpMapPoints[idx] = None
                        n_matches -= 1
        return n_matches

    # ------------------------------------------------------------------------------------------------
    # native selection of the two tracking searches (orbfe_select_f_p / _f_f, host code) when every value
    # the reference's loop compares is a double: grid query -> distances of the non-empty queries -> the
    # sequential selection in C -> the assignments (and f_f's rotation histogram) here, in order.  Returns
    # None, before touching anything, when an operand has another type (float32 projections promote
    # differently under NumPy 2): the caller then runs the Python loop.

    def _f_p_native(self, frame, pmps, lvls, rads):
        """pmps / lvls / rads: the searched map points (tracked in view, not bad), their predicted levels and
        radii; the window of each is (mTrackProjX, mTrackProjY, r * mvScaleFactors[level], level - 1,
        level) as in the reference loop."""
        grid = _frame_grid(frame)
        if grid is None or not pmps:
            return None
        if not (set(map(type, lvls)) <= _INT_SET and set(map(type, rads)) <= _F64_SET):
            return None
        sf = frame.mvScaleFactors
        if not set(map(type, sf)) <= _F64_SET:
            return None
        n = len(pmps)
        lo_hi = np.array(lvls, np.int64)
        if lo_hi.min() < -len(sf) or lo_hi.max() >= len(sf):
            return None
        qr = np.array(rads, np.float64) * np.array(sf, np.float64)[lo_hi]  # r * mvScaleFactors[level], doubles
        qx = _f64_array(list(map(_PROJ_X, pmps)))
        if qx is None:
            return None
        qy = _f64_array(list(map(_PROJ_Y, pmps)))
        if qy is None:
            return None
        xr_all = list(map(_PROJ_XR, pmps))
        xr_arr = _f64_array(xr_all)
        if xr_arr is None:
            return None
        n_frame = len(frame.mvpMapPoints)
        u_right, u_double = _u_right(frame, with_kinds=True)
        # ORBMatcher.py's er = abs(XR - mvuRight[idx]): a Python-float XR against an np.float32 entry
        # evaluates in float32 (NEP 50), which the double selection in C does not reproduce
        if not u_double and float in set(map(type, xr_all)):
            return None
        if len(u_right) != n_frame or len(grid[4]) != n_frame:
            return None
        lv32 = lo_hi.astype(np.int32)
        off, idx = _grid_csr(frame, grid, qx, qy, qr, lv32 - 1, lv32)
        rows, off2, dist = self._nonempty(off, idx, pmps, frame.mDescriptors)
        if len(rows) == 0:
            return 0
        rl = rows.tolist()
        xr = np.ascontiguousarray(xr_arr[rows])
        rs = np.ascontiguousarray(qr[rows])
        q_obs = _obs_flags(list(map(pmps.__getitem__, rl)))
        blocked = _blocked(frame)
        best = np.empty(len(rl), np.int32)
        call("orbfe_select_f_p", len(rl), ptr(off2), ptr(idx), ptr(dist), ptr(xr), ptr(rs), ptr(grid[4]), ptr(q_obs),
             ptr(u_right), ptr(blocked), n_frame, float(self.mfNNratio), TH_HIGH, ptr(best))
        hit = np.flatnonzero(best >= 0).tolist()
        # frame.mvpMapPoints[best[j]] = pmps[rl[j]] in query order, the list's own __setitem__ mapped in C
        deque(map(frame.mvpMapPoints.__setitem__, best[hit].tolist(), map(pmps.__getitem__, map(rl.__getitem__, hit))), 0)
        return len(hit)

    def _f_f_native(self, cur, last, th, b_forward, b_backward, cand, sel, u, v, invzc):
        grid = _frame_grid(cur)
        if grid is None or type(th) not in (int, float):
            return None
        if not (u.dtype == np.float64 and v.dtype == np.float64 and invzc.dtype == np.float64):
            return None
        sf = cur.mvScaleFactors
        if not all(type(x) in _F64 for x in sf):
            return None
        n_frame = len(cur.mvpMapPoints)
        u_right = _u_right(cur)
        if len(u_right) != n_frame:
            return None
        ci = np.asarray(cand, np.int64)[sel].tolist()
        octv = _octaves(last)[np.asarray(ci, np.int64)] if ci else np.zeros(0, np.int32)
        radius = th * np.asarray(sf, np.float64)[octv]  # th * mvScaleFactors[octave], one double product each
        if b_forward:
            lo, hi = octv, np.full(len(ci), -1, np.int32)
        elif b_backward:
            lo, hi = np.zeros(len(ci), np.int32), octv
        else:
            lo, hi = octv - 1, octv + 1
        qx, iz = np.ascontiguousarray(u[sel]), np.ascontiguousarray(invzc[sel])
        off, idx = _grid_csr(cur, grid, qx, v[sel], radius, lo, hi)
        pmps = list(map(last.mvpMapPoints.__getitem__, ci))
        rows, off2, dist = self._nonempty(off, idx, pmps, cur.mDescriptors)
        n_matches = 0
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        factor = 1.0 / HISTO_LENGTH
        if len(rows):
            rl = rows.tolist()
            q_obs = _obs_flags(list(map(pmps.__getitem__, rl)))
            blocked = _blocked(cur)
            best = np.empty(len(rl), np.int32)
            qu, qz, qrad = (np.ascontiguousarray(a[rows], np.float64) for a in (qx, iz, radius))  # held across the call
            call("orbfe_select_f_f", len(rl), ptr(off2), ptr(idx), ptr(dist), ptr(qu), ptr(qz), ptr(qrad), ptr(q_obs),
                 ptr(u_right), ptr(blocked), n_frame, float(cur.mbf), TH_HIGH, ptr(best))
            hit = np.flatnonzero(best >= 0)
            bl = best[hit].tolist()
            # cur.mvpMapPoints[b] = pmps[rl[j]] in query order, the list's own __setitem__ mapped in C
            deque(map(cur.mvpMapPoints.__setitem__, bl, map(pmps.__getitem__, map(rl.__getitem__, hit.tolist()))), 0)
            n_matches += len(bl)
            if self.mbCheckOrientation and bl:  # ORBMatcher.py:374-382
                la, ca = _angles(last), _angles(cur)
                if la is not None and ca is not None:  # doubles: the same arithmetic over arrays
                    rot = la[np.asarray(ci, np.int64)[rows[hit]]] - ca[best[hit]]
                    rot = np.where(rot < 0.0, rot + 360.0, rot)
                    bins = np.round(rot * factor).astype(np.int64)  # round() of a double: half to even
                    bins[bins == HISTO_LENGTH] = 0
                    bins = bins.tolist()
                else:
                    bins = []
                    for j, b in zip(hit.tolist(), bl):
                        rot = last.mvKeysUn[ci[rl[j]]].angle - cur.mvKeysUn[b].angle
                        if rot < 0.0:
                            rot += 360.0
                        bin_idx = round(rot * factor)
                        bins.append(0 if bin_idx == HISTO_LENGTH else bin_idx)
                assert not bins or 0 <= min(bins) <= max(bins) < HISTO_LENGTH  # ORBMatcher.py's per-bin assert
                for b, k in zip(bl, bins):
                    rot_hist[k].append(b)
        if self.mbCheckOrientation:
            ind1, ind2, ind3 = self.compute_three_maxima(rot_hist, HISTO_LENGTH)
            for i in range(HISTO_LENGTH):
                if i not in (ind1, ind2, ind3):
                    for idx2 in rot_hist[i]:
                        cur.mvpMapPoints[idx2] = None
                        n_matches -= 1
        return n_matches

    # ------------------------------------------------------------------------------------------------
    # helpers shared by the keyframe-level searches

    def _reject_by_rotation(self, rot_hist, on_reject):
        """Keep the three fullest rotation bins (ORBMatcher.py:16-19 + the callers' loops)."""
        ind1, ind2, ind3 = self.compute_three_maxima(rot_hist, HISTO_LENGTH)
        n = 0
        for i in range(HISTO_LENGTH):
            if i in [ind1, ind2, ind3]:
                continue
            for idx in rot_hist[i]:
                on_reject(idx)
                n += 1
        return n

    @staticmethod
    def _bow_common_nodes(fv1, fv2):
        """Nodes present in both DBoW2 feature vectors, in the order the reference's merge walk visits
        them (ORBMatcher.py:39-103, 140-196: advance both on equal keys, else the smaller one)."""
        out = []
        it1, it2 = iter(fv1), iter(fv2)
        try:
            k1 = next(it1)
            k2 = next(it2)
            while True:
                if k1 == k2:
                    out.append(k1)
                    k1 = next(it1)
                    k2 = next(it2)
                elif k1 < k2:
                    k1 = next(it1)
                else:
                    k2 = next(it2)
        except StopIteration:
            pass
        return out

    def _query_dists(self, pMP, snap, cands, dq, train):
        """Distances of a query collected earlier; re-run on the GPU if its descriptor changed since."""
        d = pMP.get_descriptor()
        if np.array_equal(np.asarray(d).reshape(-1), np.asarray(snap).reshape(-1)):
            return dq
        return self._batched([(d, cands)], train)[0]

    # ORBMatcher.py:21-118
    def search_by_BoW_kf_f(self, kf, frame):
        vpMapPointsKF = kf.get_map_point_matches()
        vpMapPointMatches = [None] * frame.N
        fv_kf, fv_f = kf.mFeatVec, frame.mFeatVec
        n_matches = 0
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        factor = 1.0 / HISTO_LENGTH
        work = []
        for node in self._bow_common_nodes(fv_kf, fv_f):
            cands = fv_f[node]
            for idx_kf in fv_kf[node]:
                pMP = vpMapPointsKF[idx_kf]
                if not pMP or pMP.is_bad():
                    continue
                work.append((idx_kf, pMP, cands, kf.mDescriptors[idx_kf]))
        dists = self._batched([(w[3], w[2]) for w in work], frame.mDescriptors)
        for (idx_kf, pMP, cands, _), dq in zip(work, dists):
            best1, best_idx, best2 = 256, -1, 256
            for idx_f, dist in zip(cands, dq.tolist()):
                if vpMapPointMatches[idx_f]:
                    continue
                if dist < best1:
                    best2 = best1
                    best1 = dist
                    best_idx = idx_f
                elif dist < best2:
                    best2 = dist
            if best1 <= TH_LOW and float(best1) < self.mfNNratio * float(best2):
                vpMapPointMatches[best_idx] = pMP
                kp = kf.mvKeysUn[idx_kf]
                if self.mbCheckOrientation:
                    rot = kp.angle - frame.mvKeys[best_idx].angle
                    if rot < 0.0:
                        rot += 360.0
                    b = round(rot * factor)
                    if b == HISTO_LENGTH:
                        b = 0
                    assert 0 <= b < HISTO_LENGTH
                    rot_hist[b].append(best_idx)
                n_matches += 1
        if self.mbCheckOrientation:
            n_matches -= self._reject_by_rotation(rot_hist, lambda i: vpMapPointMatches.__setitem__(i, None))
        return n_matches, vpMapPointMatches

    # ORBMatcher.py:120-213
    def search_by_BoW_kf_kf(self, pKF1, pKF2):
        vKeysUn1, vKeysUn2 = pKF1.mvKeysUn, pKF2.mvKeysUn
        fv1, fv2 = pKF1.mFeatVec, pKF2.mFeatVec
        vpMapPoints1 = pKF1.get_map_point_matches()
        vpMapPoints2 = pKF2.get_map_point_matches()
        vpMatches12 = [None] * len(vpMapPoints1)
        vbMatched2 = [False] * len(vpMapPoints2)
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        factor = 1.0 / HISTO_LENGTH
        n_matches = 0
        work = []
        for node in self._bow_common_nodes(fv1, fv2):
            cands = []
            for idx2 in fv2[node]:
                pMP2 = vpMapPoints2[idx2]
                if not pMP2 or pMP2.is_bad():
                    continue
                cands.append(idx2)
            for idx1 in fv1[node]:
                pMP1 = vpMapPoints1[idx1]
                if not pMP1 or pMP1.is_bad():
                    continue
                work.append((idx1, cands, pKF1.mDescriptors[idx1]))
        dists = self._batched([(w[2], w[1]) for w in work], pKF2.mDescriptors)
        for (idx1, cands, _), dq in zip(work, dists):
            best1, best_idx2, best2 = 256, -1, 256
            for idx2, dist in zip(cands, dq.tolist()):
                if vbMatched2[idx2]:
                    continue
                if dist < best1:
                    best2 = best1
                    best1 = dist
                    best_idx2 = idx2
                elif dist < best2:
                    best2 = dist
            if best1 < TH_LOW and best1 < self.mfNNratio * best2:
                vpMatches12[idx1] = vpMapPoints2[best_idx2]
                vbMatched2[best_idx2] = True
                if self.mbCheckOrientation:
                    rot = vKeysUn1[idx1].angle - vKeysUn2[best_idx2].angle
                    if rot < 0.0:
                        rot += 360.0
                    b = round(rot * factor)
                    if b == HISTO_LENGTH:
                        b = 0
                    rot_hist[b].append(idx1)
                n_matches += 1
        if self.mbCheckOrientation:
            n_matches -= self._reject_by_rotation(rot_hist, lambda i: vpMatches12.__setitem__(i, None))
        return n_matches, vpMatches12

    # ------------------------------------------------------------------------------------------------
    # the two BoW searches for many candidates at once: one k_bow_match launch (orbfe_bow_match)

    def _bow_many(self, frames, pairs, inclusive, elig2):
        """One launch over array forms of `frames` (None where a frame has none); pairs (a, b) index frames.
        Returns per pair None (an operand the arrays cannot express: the caller takes the single search) or
        (match12, match21, n) after the rotation rejection."""
        ratio = self.mfNNratio
        ok = type(ratio) in _DOUBLE_OR_INT_SET
        live = [p for p, (a, b) in enumerate(pairs) if ok and frames[a] is not None and frames[b] is not None]
        out = [None] * len(pairs)
        if not live:
            return out
        used = sorted({f for p in live for f in pairs[p]})
        slot = {f: k for k, f in enumerate(used)}
        fa = [frames[f] for f in used]
        off = np.zeros(len(fa) + 1, np.int64)
        np.cumsum([len(f.desc) for f in fa], out=off[1:])
        fv_off = np.zeros(len(fa) + 1, np.int64)
        np.cumsum([len(f.fv_node) for f in fa], out=fv_off[1:])
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dt) if xs else np.zeros(0, dt)  # noqa: E731
        fv_idx = np.zeros(int(off[-1]), np.int32)
        for k, f in enumerate(fa):
            fv_idx[off[k]:off[k] + len(f.fv_idx)] = f.fv_idx
        elig = cat([f.elig for f in fa], np.uint8)
        r = bow_match_arrays(cat([f.desc for f in fa], np.uint8).reshape(-1, 32), cat([f.angle for f in fa], np.float32),
                             off, fv_off, cat([f.fv_node for f in fa], np.int32), cat([f.fv_end for f in fa], np.int32),
                             fv_idx, np.array([[slot[a], slot[b]] for a, b in (pairs[p] for p in live)], np.int32),
                             TH_LOW, inclusive, float(ratio), elig, elig if elig2 else None)
        for k, p in enumerate(live):
            n1, n2 = len(frames[pairs[p][0]].desc), len(frames[pairs[p][1]].desc)
            if r["hist"][k, HISTO_LENGTH:].any():  # an angle outside [0, 360]: the reference's own indexing decides
                continue
            out[p] = self._bow_reject(r["match12"][k, :n1], r["match21"][k, :n2], r["bin12"][k, :n1], r["hist"][k],
                                      int(r["n_raw"][k]))
        return out

    def _bow_reject(self, match12, match21, bin12, hist, n_raw):
        """The rotation rejection of the BoW searches over k_bow_match's raw outputs (ORBMatcher.py:108-116,
        202-210): compute_three_maxima on the histogram, as the reference ranks it on this host."""
        if not self.mbCheckOrientation:
            return match12, match21, n_raw
        keep = np.zeros(HISTO_LENGTH + 2, bool)
        keep[np.asarray(self.compute_three_maxima([range(c) for c in hist[:HISTO_LENGTH].tolist()], HISTO_LENGTH))] = True
        drop = (match12 >= 0) & ~keep[bin12]
        match12, match21 = match12.copy(), match21.copy()
        match21[match12[drop]] = -1
        match12[drop] = -1
        return match12, match21, n_raw - int(drop.sum())

    def search_by_BoW_kf_kf_many(self, pKF1, kfs2):
        """[search_by_BoW_kf_kf(pKF1, kf) for kf in kfs2] (LoopClosing.compute_sim3's loop, LoopClosing.py:156-166),
        value for value, with one launch for the whole list."""
        kfs2 = list(kfs2)
        vps = [pKF1.get_map_point_matches()] + [kf.get_map_point_matches() for kf in kfs2]
        frames = [_bow_frame(kf, kf.mvKeysUn, vp) for kf, vp in zip([pKF1] + kfs2, vps)]
        res = self._bow_many(frames, [(0, j + 1) for j in range(len(kfs2))], False, True)
        out = []
        for j, (kf, r) in enumerate(zip(kfs2, res)):
            if r is None:
                out.append(self.search_by_BoW_kf_kf(pKF1, kf))
                continue
            m12 = r[0].tolist()
            vp2 = vps[j + 1]
            out.append((r[2], [vp2[i2] if i2 >= 0 else None for i2 in m12]))
        return out

    def search_by_BoW_kf_f_many(self, kfs, frame):
        """[search_by_BoW_kf_f(kf, frame) for kf in kfs] (Tracking.relocalization's loop, Tracking.py:677-685),
        value for value, with one launch for the whole list."""
        kfs = list(kfs)
        vps = [kf.get_map_point_matches() for kf in kfs]
        frames = [_bow_frame(kf, kf.mvKeysUn, vp) for kf, vp in zip(kfs, vps)]
        fr = _bow_frame(frame, frame.mvKeys, None)
        if fr is not None and len(fr.desc) != frame.N:
            fr = None
        frames.append(fr)
        res = self._bow_many(frames, [(j, len(kfs)) for j in range(len(kfs))], True, False)
        out = []
        for kf, vp, r in zip(kfs, vps, res):
            if r is None:
                out.append(self.search_by_BoW_kf_f(kf, frame))
                continue
            out.append((r[2], [vp[i1] if i1 >= 0 else None for i1 in r[1].tolist()]))
        return out

    @staticmethod
    def _sim3_to_pose(Scw):
        sRcw = Scw[:3, :3]
        scw = np.sqrt(np.dot(sRcw[0], sRcw[0]))
        Rcw = sRcw / scw
        tcw = Scw[:3, 3:4] / scw
        return Rcw, tcw, -Rcw.T @ tcw

    @staticmethod
    def _project_checked(pMP, pKF, Rcw, tcw, strict_z):
        """Camera projection of fuse_kf_scw_mp (:414-427, strict_z False) and
        search_by_projection_ckf_scw_mp (:868-878, strict_z True: `<= 0` and 1-element array
        arithmetic, as there).  Returns (u, v, invz, p3Dw) or None."""
        p3Dw = pMP.get_world_pos()
        p3Dc = Rcw @ p3Dw + tcw
        if strict_z:
            if p3Dc[2][0] <= 0.0:
                return None
            invz = 1.0 / p3Dc[2]
            x, y = p3Dc[0] * invz, p3Dc[1] * invz
        else:
            if p3Dc[2][0] < 0.0:
                return None
            invz = 1.0 / p3Dc[2][0]
            x = p3Dc[0][0] * invz
            y = p3Dc[1][0] * invz
        u = pKF.fx * x + pKF.cx
        v = pKF.fy * y + pKF.cy
        return u, v, invz, p3Dw

    @staticmethod
    def _distance_gates(pMP, pKF, p3Dw, Ow):
        """Scale-invariance distance and viewing-angle gates (:429-441); the predicted level or None."""
        maxDistance = pMP.get_max_distance_invariance()
        minDistance = pMP.get_min_distance_invariance()
        PO = p3Dw - Ow
        dist3D = np.linalg.norm(PO)
        if dist3D < minDistance or dist3D > maxDistance:
            return None
        Pn = pMP.get_normal()
        if np.dot(PO.T, Pn) < 0.5 * dist3D:
            return None
        return pMP.predict_scale(dist3D, pKF)

    # ORBMatcher.py:395-480
    def fuse_kf_scw_mp(self, pKF, Scw, vpPoints, th, vpReplacePoint):
        Rcw, tcw, Ow = self._sim3_to_pose(Scw)
        spAlreadyFound = pKF.get_map_points()
        work = []
        for iMP, pMP in enumerate(vpPoints):
            if pMP.is_bad() or pMP in spAlreadyFound:
                continue
            pr = self._project_checked(pMP, pKF, Rcw, tcw, False)
            if pr is None:
                continue
            u, v, _, p3Dw = pr
            if not pKF.is_in_image(u, v):
                continue
            lvl = self._distance_gates(pMP, pKF, p3Dw, Ow)
            if lvl is None:
                continue
            vIndices = pKF.get_features_in_area(u, v, th * pKF.mvScaleFactors[lvl])
            if not vIndices:
                continue
            cands = [i for i in vIndices if lvl - 1 <= pKF.mvKeysUn[i].octave <= lvl]
            work.append((iMP, pMP, cands, pMP.get_descriptor()))
        dists = self._batched([(w[3], w[2]) for w in work], pKF.mDescriptors)
        n_fused = 0
        for (iMP, pMP, cands, _), dq in zip(work, dists):
            best_dist, best_idx = float('inf'), -1
            for idx, dist in zip(cands, dq.tolist()):
                if dist < best_dist:
                    best_dist = dist
                    best_idx = idx
            if best_dist <= TH_LOW:
                pMPinKF = pKF.get_map_point(best_idx)
                if pMPinKF:
                    if not pMPinKF.is_bad():
                        vpReplacePoint[iMP] = pMPinKF
                else:
                    pMP.add_observation(pKF, best_idx)
                    pKF.add_map_point(pMP, best_idx)
                n_fused += 1
        return n_fused, vpReplacePoint

    def _scw_one(self, pKF, pMP, Rcw, tcw, Ow, th, vpMatched=None):
        """(best_dist, best_idx) of one point in one keyframe with the reference's own expressions on the objects:
        ORBMatcher.py:415-468 (fuse_kf_scw_mp) when vpMatched is None, :867-916 (search_by_projection_ckf_scw_mp)
        against that vpMatched otherwise; the few distances are host popcounts.  best_idx is -1 without a
        candidate."""
        ckf = vpMatched is not None
        best_dist, best_idx = (256 if ckf else float('inf')), -1
        pr = self._project_checked(pMP, pKF, Rcw, tcw, ckf)
        if pr is None:
            return best_dist, best_idx
        u, v, _, p3Dw = pr
        if not pKF.is_in_image(u, v):
            return best_dist, best_idx
        lvl = self._distance_gates(pMP, pKF, p3Dw, Ow)
        if lvl is None:
            return best_dist, best_idx
        vIndices = pKF.get_features_in_area(u, v, th * pKF.mvScaleFactors[lvl])
        if not vIndices:
            return best_dist, best_idx
        d = pMP.get_descriptor()
        for idx in vIndices:
            if ckf and vpMatched[idx] is not None:
                continue
            if not lvl - 1 <= pKF.mvKeysUn[idx].octave <= lvl:
                continue
            dist = descriptor_distance(d, pKF.mDescriptors[idx])
            if dist < best_dist:
                best_dist = dist
                best_idx = idx
        return best_dist, best_idx

    @staticmethod
    def _scw_frame(pKF, Scw, pose):
        """(_FuseFrame of pKF with the pose slots filled from Scw, (Rcw, tcw, Ow) as pose(Scw) gave them), or None
        when _fuse_frame refuses the keyframe, when Scw is not a finite 4 x 4 float32 / float64 array with a non-zero
        first row, or when the pose it gives is not finite.  f.f32 tells whether Scw is float32."""
        if not (type(Scw) is np.ndarray and Scw.shape == (4, 4) and Scw.dtype in _POSE_DT
                and bool(np.isfinite(Scw).all()) and bool(Scw[0, :3].any())):
            return None
        f = _fuse_frame(pKF)
        if f is None:
            return None
        with np.errstate(all="ignore"):
            Rcw, tcw, Ow = pose(Scw)
        R, t, O = _pose_part(Rcw, (3, 3)), _pose_part(tcw, (3, 1)), _pose_part(Ow, (3, 1))
        if R is None or t is None or O is None:
            return None
        f.f64 = f.f64.copy()
        f.f64[5:20] = R[0] + t[0] + O[0]
        f.f32 = Scw.dtype == _F32_DT
        return f, (Rcw, tcw, Ow)

    @staticmethod
    def _search_points(vpPoints, skip, normal=True, f32_dist=False):
        """The points once: (slot per list position, rows, descriptor rows, any float32).  slot >= 0 is the row sent
        to the device, -1 not expressible (_fuse_point, with its normal), -2 skipped by skip(pMP)."""
        slot, rows, descs, f32 = [], [], [], False
        for pMP in vpPoints:
            if skip(pMP):
                slot.append(-2)
                continue
            pt = _fuse_point(pMP, normal, f32_dist)
            if pt is None:
                slot.append(-1)
                continue
            slot.append(len(rows))
            rows.append(pt[0])
            descs.append(pt[1])
            f32 = f32 or pt[2]
        return slot, rows, descs, f32

    @staticmethod
    def _search_launch(fr, rows, descs, th, f32, fuse=False, blocked=None, sim3=None, fkf=None, local=None, ff=None):
        """The frames fr and the points (rows, descs) packed into one call of fuse_search_arrays (fuse), of
        scw_search_arrays (with blocked), of sim3_search_arrays (with sim3 = (srch_f64, srch_kf, srch_off,
        item_pt)), of fkf_search_arrays (with blocked and fkf = (srch_kf, srch_off, item_pt)) or of
        local_search_arrays (with blocked and local = (srch_limit, srch_kf, srch_off, item_pt, th_on)) or of
        ff_search_arrays (with blocked and ff = (srch_th, srch_mode, srch_kf, srch_off, item_pt, item_level))."""
        def offs(lens):
            o = np.zeros(len(fr) + 1, np.int64)
            np.cumsum(lens, out=o[1:])
            return o
        cat = lambda name: np.concatenate([getattr(f, name) for f in fr])  # noqa: E731
        head = (np.stack([f.f64 for f in fr]), np.stack([f.i32 for f in fr]), offs([len(f.xy) for f in fr]), cat("xy"),
                cat("octave"))
        grid = (offs([len(f.cell_off) for f in fr]), cat("cell_off"), offs([len(f.cell_idx) for f in fr]),
                cat("cell_idx"), offs([len(f.scale) for f in fr]), cat("scale"))
        # descriptor rows already stacked (an (n, 32) array) stand as they are
        pts = (np.array(rows, np.float64), descs if type(descs) is np.ndarray and descs.ndim == 2 else np.stack(descs),
               th, FUSE_EPS_F32 if f32 else FUSE_EPS_F64)
        if fuse:
            return fuse_search_arrays(*head, cat("u_right"), cat("desc"), *grid, cat("inv_sigma2"), *pts)
        if sim3 is not None:
            return sim3_search_arrays(*head, cat("desc"), *grid, *pts[:2], *sim3, *pts[2:])
        if fkf is not None:
            return fkf_search_arrays(*head, cat("desc"), blocked, *grid, *pts[:2], *fkf, *pts[2:])
        if local is not None:
            return local_search_arrays(*head, cat("u_right"), cat("desc"), blocked, *grid, *pts[:2], *local[:4], th,
                                       local[4], pts[3])
        if ff is not None:
            return ff_search_arrays(*head, cat("u_right"), cat("desc"), blocked, *grid, *pts[:2], *ff, pts[3])
        return scw_search_arrays(*head, cat("desc"), blocked, *grid, *pts)

    def fuse_kf_scw_mp_many(self, kfs, Scws, vpPoints, th, after=None):
        """What this loop returns (LoopClosing.search_and_fuse, LoopClosing.py:352-367, with after = its replace
        loop), leaving every map point and keyframe as the loop leaves them, event for event, from one k_scw_search
        launch for every (keyframe, point) of the call:

            out = []
            for kf, Scw in zip(kfs, Scws):
                r = self.fuse_kf_scw_mp(kf, Scw, vpPoints, th, [None] * len(vpPoints))
                if after is not None:
                    after(kf, r[1])
                out.append(r)

        Per keyframe Rcw, tcw and Ow come from _sim3_to_pose(Scw), the reference's own expressions on the host.  The
        points are read once: every point that is not bad and that the arrays can express (_fuse_point).  The replay
        runs keyframe by keyframe; at a keyframe's turn spAlreadyFound = kf.get_map_points() is the snapshot of that
        moment, as the reference's is, and then point by point in list order with is_bad() read at that moment.
        ORBMatcher.py:470-478 is applied to the device's best candidate, get_map_point(best_idx) read at that moment,
        so a point added earlier in the same pass is seen.  One item is redone alone with the reference's
        expressions (_scw_one) when it came back ORBFE_FUSE_MARGINAL, when its point is not expressible, or when
        its point's descriptor is no longer the bytes that were sent (MapPoint.replace recomputes the survivor's).
        A keyframe _fuse_frame refuses takes fuse_kf_scw_mp whole at its place in the order, as does one whose Scw
        is not a finite 4 x 4 float32 / float64 array with a non-zero first row, and every keyframe when th is not a
        plain finite number.

        after(kf, vpReplacePoint) runs after each keyframe.  It may replace points, add observations and make
        points bad, which is what search_and_fuse does; it must not move points or change the level tables or grids
        of keyframes still to come, which were read before the first keyframe's turn."""
        kfs, Scws = list(kfs), list(Scws)
        if len(kfs) != len(Scws):
            raise ValueError("one Scw per keyframe")
        if not isinstance(vpPoints, (list, tuple)):
            vpPoints = list(vpPoints)
        n_pts = len(vpPoints)

        def whole(kf, Scw):
            r = self.fuse_kf_scw_mp(kf, Scw, vpPoints, th, [None] * n_pts)
            if after is not None:
                after(kf, r[1])
            return r
        if type(th) not in _TH_SET or not np.isfinite(th):
            return [whole(kf, Scw) for kf, Scw in zip(kfs, Scws)]
        frames = [self._scw_frame(kf, Scw, self._sim3_to_pose) for kf, Scw in zip(kfs, Scws)]
        live = [k for k, f in enumerate(frames) if f is not None]
        slot, rows, descs, f32 = self._search_points(vpPoints, _IS_BAD) if live else ([], [], [], False)
        res, snaps = None, []
        if live and rows:
            fr = [frames[k][0] for k in live]
            snaps = [d.tobytes() for d in descs]
            res = self._search_launch(fr, rows, descs, th, f32 or any(f.f32 for f in fr))
        slot_arr = np.array(slot, np.int64)
        alone = np.flatnonzero(slot_arr == -1)   # list positions whose point goes alone in every keyframe
        sent = np.flatnonzero(slot_arr >= 0)     # list positions in device row order
        row = {k: j for j, k in enumerate(live)}
        out = []
        for k, (kf, Scw) in enumerate(zip(kfs, Scws)):
            if frames[k] is None:
                out.append(whole(kf, Scw))
                continue
            Rcw, tcw, Ow = frames[k][1]
            if res is None:
                todo, bi, bd, st = alone, None, None, None
            else:
                j = row[k]
                bi, bd, st = res["best_idx"][j], res["best_dist"][j], res["status"][j]
                # an item without a candidate and without a marginal decision does nothing, whatever its
                # descriptor has become; the others in list order
                todo = np.sort(np.concatenate([alone, sent[(bi >= 0) | (st != 0)]]))
                bi, bd, st = bi.tolist(), bd.tolist(), st.tolist()
            spAlreadyFound = kf.get_map_points()
            rep = [None] * n_pts
            n_fused = 0
            for i in todo.tolist():
                pMP = vpPoints[i]
                if pMP.is_bad() or pMP in spAlreadyFound:
                    continue
                s = slot[i]
                if s >= 0 and not st[s] and pMP.get_descriptor().tobytes() == snaps[s]:
                    best_dist, best_idx = bd[s], bi[s]
                else:
                    best_dist, best_idx = self._scw_one(kf, pMP, Rcw, tcw, Ow, th)
                if best_idx >= 0 and best_dist <= TH_LOW:
                    pMPinKF = kf.get_map_point(best_idx)
                    if pMPinKF:
                        if not pMPinKF.is_bad():
                            rep[i] = pMPinKF
                    else:
                        pMP.add_observation(kf, best_idx)
                        kf.add_map_point(pMP, best_idx)
                    n_fused += 1
            if after is not None:
                after(kf, rep)
            out.append((n_fused, rep))
        return out

    def _fuse_cands(self, pKF, pMP, th, K):
        """The search of fuse_pkf_mp for one point, up to the descriptor distances (ORBMatcher.py:498-560): the
        candidates that pass the octave filter and the chi-square, in visiting order, or None when the point is
        skipped before the candidates are read.  K: (fx, fy, cx, cy, bf, Rcw, tcw, Ow) of the keyframe."""
        fx, fy, cx, cy, bf, Rcw, tcw, Ow = K
        p3Dw = pMP.get_world_pos()
        p3Dc = Rcw @ p3Dw + tcw
        if p3Dc[2][0] < 0.0:
            return None
        invz = 1.0 / p3Dc[2][0]
        x = p3Dc[0][0] * invz
        y = p3Dc[1][0] * invz
        u = fx * x + cx
        v = fy * y + cy
        ur = u - bf * invz
        if not pKF.is_in_image(u, v):
            return None
        lvl = self._distance_gates(pMP, pKF, p3Dw, Ow)
        if lvl is None:
            return None
        vIndices = pKF.get_features_in_area(u, v, th * pKF.mvScaleFactors[lvl])
        if not vIndices:
            return None
        cands = []
        for idx in vIndices:
            kp = pKF.mvKeysUn[idx]
            kpLevel = kp.octave
            if kpLevel < lvl - 1 or kpLevel > lvl:
                continue
            if pKF.mvuRight[idx] >= 0:
                ex, ey, er = u - kp.pt[0], v - kp.pt[1], ur - pKF.mvuRight[idx]
                if (ex ** 2 + ey ** 2 + er ** 2) * pKF.mvInvLevelSigma2[kpLevel] > 7.8:
                    continue
            else:
                ex, ey = u - kp.pt[0], v - kp.pt[1]
                if (ex ** 2 + ey ** 2) * pKF.mvInvLevelSigma2[kpLevel] > 5.99:
                    continue
            cands.append(idx)
        return cands

    @staticmethod
    def _fuse_apply(pKF, pMP, best_idx):
        """ORBMatcher.py:570-579: what fuse_pkf_mp does with a point's best candidate."""
        pMPinKF = pKF.get_map_point(best_idx)
        if pMPinKF:
            if not pMPinKF.is_bad():
                if pMPinKF.observations() > pMP.observations():
                    pMP.replace(pMPinKF)
                else:
                    pMPinKF.replace(pMP)
        else:
            pMP.add_observation(pKF, best_idx)
            pKF.add_map_point(pMP, best_idx)

    # ORBMatcher.py:482-582
    def fuse_pkf_mp(self, pKF, vpMapPoints, th):
        K = (pKF.fx, pKF.fy, pKF.cx, pKF.cy, pKF.mbf, pKF.get_rotation(), pKF.get_translation(),
             pKF.get_camera_center())
        work = []
        for pMP in vpMapPoints:
            # badness never reverts, so a point bad now is skipped by the replay as well; whether it is in
            # the keyframe can change during the search and is checked there
            if not pMP or pMP.is_bad():
                continue
            cands = self._fuse_cands(pKF, pMP, th, K)
            if cands is None:
                continue
            work.append((pMP, cands, pMP.get_descriptor()))
        dists = self._batched([(w[2], w[1]) for w in work], pKF.mDescriptors)
        n_fused = 0
        for (pMP, cands, snap), dq in zip(work, dists):
            if pMP.is_bad() or pMP.is_in_key_frame(pKF):
                continue
            dq = self._query_dists(pMP, snap, cands, dq, pKF.mDescriptors)
            best_dist, best_idx = float('inf'), -1
            for idx, dist in zip(cands, dq.tolist()):
                if dist < best_dist:
                    best_dist = dist
                    best_idx = idx
            if best_dist <= TH_LOW:
                self._fuse_apply(pKF, pMP, best_idx)
                n_fused += 1
        return n_fused

    def _fuse_one(self, pKF, pMP, th, K):
        """(best_dist, best_idx) of one point in one keyframe with the reference's own expressions on the objects
        (ORBMatcher.py:498-567); the few distances are host popcounts.  (inf, -1) without a candidate."""
        cands = self._fuse_cands(pKF, pMP, th, K)
        best_dist, best_idx = float('inf'), -1
        if cands:
            d = pMP.get_descriptor()
            for idx in cands:
                dist = descriptor_distance(d, pKF.mDescriptors[idx])
                if dist < best_dist:
                    best_dist = dist
                    best_idx = idx
        return best_dist, best_idx

    def fuse_pkf_mp_many(self, kfs, vpMapPoints, th):
        """[fuse_pkf_mp(kf, vpMapPoints, th) for kf in kfs] (LocalMapping.search_in_neighbors' loops,
        LocalMapping.py:359-360 and :375), value for value and side effect for side effect, with one k_fuse_search
        launch for every (keyframe, point) of the call.  The points are read once: every point that is not None, not
        bad and that the arrays can express (_fuse_point).  The replay then runs on the host in the reference's
        order, keyframe by keyframe and point by point, with is_bad() and is_in_key_frame(kf) read at that moment,
        and applies ORBMatcher.py:569-580 to the device's best candidate.  One item is redone alone with the
        reference's expressions (_fuse_one) when it came back ORBFE_FUSE_MARGINAL, when its point is not
        expressible, or when its point's descriptor is no longer the one that was sent (MapPoint.replace recomputes
        the survivor's).  A keyframe _fuse_frame refuses takes fuse_pkf_mp whole at its place in the order, as does
        every keyframe when th is not a plain number."""
        kfs = list(kfs)
        if not isinstance(vpMapPoints, (list, tuple)):
            vpMapPoints = list(vpMapPoints)
        if type(th) not in _TH_SET or not np.isfinite(th):
            return [self.fuse_pkf_mp(kf, vpMapPoints, th) for kf in kfs]
        frames = [_fuse_frame(kf) for kf in kfs]
        live = [k for k, f in enumerate(frames) if f is not None]
        # the points once (slot -2: None or bad already), and none when no keyframe is expressible
        skip = lambda p: not p or p.is_bad()  # noqa: E731
        slot, rows, descs, f32 = self._search_points(vpMapPoints, skip) if live else ([], [], [], False)
        res, snaps = None, []
        if live and rows:
            fr = [frames[k] for k in live]
            snaps = [d.tobytes() for d in descs]
            res = self._search_launch(fr, rows, descs, th, f32 or any(f.f32 for f in fr), fuse=True)
        slot_arr = np.array(slot, np.int64)
        alone = np.flatnonzero(slot_arr == -1)   # list positions whose point goes alone in every keyframe
        sent = np.flatnonzero(slot_arr >= 0)     # list positions in device row order
        out = []
        row = {k: j for j, k in enumerate(live)}
        for k, kf in enumerate(kfs):
            if frames[k] is None:
                out.append(self.fuse_pkf_mp(kf, vpMapPoints, th))
                continue
            if res is None:
                todo, bi, bd, st = alone, None, None, None
            else:
                j = row[k]
                bi, bd, st = res["best_idx"][j], res["best_dist"][j], res["status"][j]
                # an item without a candidate and without a marginal decision does nothing, whatever its
                # descriptor has become; the others in list order
                todo = np.sort(np.concatenate([alone, sent[(bi >= 0) | (st != 0)]]))
                bi, bd, st = bi.tolist(), bd.tolist(), st.tolist()
            K = None
            n_fused = 0
            for i in todo.tolist():
                pMP = vpMapPoints[i]
                if pMP.is_bad() or pMP.is_in_key_frame(kf):
                    continue
                s = slot[i]
                if s >= 0 and not st[s] and pMP.get_descriptor().tobytes() == snaps[s]:
                    best_dist, best_idx = bd[s], bi[s]
                else:
                    if K is None:
                        K = (kf.fx, kf.fy, kf.cx, kf.cy, kf.mbf, kf.get_rotation(), kf.get_translation(),
                             kf.get_camera_center())
                    best_dist, best_idx = self._fuse_one(kf, pMP, th, K)
                if best_idx >= 0 and best_dist <= TH_LOW:
                    self._fuse_apply(kf, pMP, best_idx)
                    n_fused += 1
            out.append(n_fused)
        return out

    @staticmethod
    def _triangulation_nodes(fv1, fv2):
        """The node pairs search_for_triangulation visits (ORBMatcher.py:606-675).  Its walk draws a
        fresh item from both vectors every round and, on unequal keys, discards one more item of the
        smaller side — outside the try block, so an exhausted vector there raises StopIteration out of
        the search.  Reproduced as is (the search has no side effects before that point)."""
        out = []
        it1, it2 = iter(fv1.items()), iter(fv2.items())
        while True:
            try:
                k1, v1 = next(it1)
                k2, v2 = next(it2)
            except StopIteration:
                break
            if k1 == k2:
                out.append((v1, v2))
            elif k1 < k2:
                next(it1)
            else:
                next(it2)
        return out

    # ORBMatcher.py:584-696
    def search_for_triangulation(self, pKF1, pKF2, F12, bOnlyStereo=False):
        Cw = pKF1.get_camera_center()
        R2w = pKF2.get_rotation()
        t2w = pKF2.get_translation()
        C2 = R2w @ Cw + t2w
        invz = 1.0 / C2[2]
        ex = pKF2.fx * C2[0] * invz + pKF2.cx
        ey = pKF2.fy * C2[1] * invz + pKF2.cy
        vbMatched2 = [False] * pKF2.N
        vMatches12 = [-1] * pKF1.N
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        factor = 1.0 / HISTO_LENGTH
        n_matches = 0
        work = []
        for f1val, f2val in self._triangulation_nodes(pKF1.mFeatVec, pKF2.mFeatVec):
            cands = []
            for idx2 in f2val:
                if pKF2.get_map_point(idx2):
                    continue
                bStereo2 = pKF2.mvuRight[idx2] >= 0
                if bOnlyStereo and not bStereo2:
                    continue
                cands.append((idx2, bStereo2))
            for idx1 in f1val:
                if pKF1.get_map_point(idx1):
                    continue
                bStereo1 = pKF1.mvuRight[idx1] >= 0
                if bOnlyStereo and not bStereo1:
                    continue
                work.append((idx1, bStereo1, cands, pKF1.mDescriptors[idx1]))
        dists = self._batched([(w[3], [c[0] for c in w[2]]) for w in work], pKF2.mDescriptors)
        for (idx1, bStereo1, cands, _), dq in zip(work, dists):
            kp1 = pKF1.mvKeysUn[idx1]
            best_dist, best_idx2 = TH_LOW, -1
            for (idx2, bStereo2), dist in zip(cands, dq.tolist()):
                if vbMatched2[idx2]:
                    continue
                if dist > TH_LOW or dist > best_dist:
                    continue
                kp2 = pKF2.mvKeysUn[idx2]
                if not bStereo1 and not bStereo2:
                    distex = ex - kp2.pt[0]
                    distey = ey - kp2.pt[1]
                    if distex ** 2 + distey ** 2 < 100 * pKF2.mvScaleFactors[kp2.octave]:
                        continue
                if self.check_dist_epipolar_line(kp1, kp2, F12, pKF2):
                    best_idx2 = idx2
                    best_dist = dist
            if best_idx2 >= 0:
                kp2 = pKF2.mvKeysUn[best_idx2]
                vMatches12[idx1] = best_idx2
                n_matches += 1
                vbMatched2[best_idx2] = True
                if self.mbCheckOrientation:
                    rot = kp1.angle - kp2.angle
                    if rot < 0:
                        rot += 360.0
                    b = round(rot * factor)
                    if b == HISTO_LENGTH:
                        b = 0
                    rot_hist[b].append(idx1)
        if self.mbCheckOrientation:
            n_matches -= self._reject_by_rotation(rot_hist, lambda i: vMatches12.__setitem__(i, -1))
        return [(i, m) for i, m in enumerate(vMatches12) if m >= 0]

    # ORBMatcher.py:698-711
    def check_dist_epipolar_line(self, kp1, kp2, F12, pKF2):
        a = kp1.pt[0] * F12[0, 0] + kp1.pt[1] * F12[1, 0] + F12[2, 0]
        b = kp1.pt[0] * F12[0, 1] + kp1.pt[1] * F12[1, 1] + F12[2, 1]
        c = kp1.pt[0] * F12[0, 2] + kp1.pt[1] * F12[1, 2] + F12[2, 2]
        num = a * kp2.pt[0] + b * kp2.pt[1] + c
        den = a ** 2 + b ** 2
        if den == 0:
            return False
        return (num ** 2) / den < 3.84 * pKF2.mvLevelSigma2[kp2.octave]

    # ------------------------------------------------------------------------------------------------
    # search_for_triangulation for many neighbours at once: one k_tri_match launch (orbfe_tri_match)

    def search_for_triangulation_many(self, pKF1, kfs2, F12s, bOnlyStereo=False):
        """[search_for_triangulation(pKF1, kf, F, bOnlyStereo) for kf, F in zip(kfs2, F12s)]
        (LocalMapping.create_new_map_points' loop, LocalMapping.py:152-183), list for list, with one launch for the
        whole list.  An element the arrays cannot express (_tri_frame, an F12 that is not a 3 x 3 float64 array,
        an epipole _tri_epipole refuses) or that comes back ORBFE_TRI_MARGINAL takes the single search; where the
        reference's walk lets StopIteration escape at element j, it is raised here after the elements before j."""
        todo = list(zip(kfs2, F12s))
        f1 = _tri_frame(pKF1)
        frames, live, F, epi = [f1], [], [], []
        for j, (kf, F12) in enumerate(todo):
            if f1 is None:
                break
            if not (type(F12) is np.ndarray and F12.shape == (3, 3) and F12.dtype == _F64_DT
                    and bool(np.isfinite(F12).all())):
                continue
            f2 = f1 if kf is pKF1 else _tri_frame(kf)
            if f2 is None:
                continue
            # the epipole with the reference's own expressions (ORBMatcher.py:589-595)
            Cw = pKF1.get_camera_center()
            R2w = kf.get_rotation()
            t2w = kf.get_translation()
            C2 = R2w @ Cw + t2w
            invz = 1.0 / C2[2]
            ex = kf.fx * C2[0] * invz + kf.cx
            ey = kf.fy * C2[1] * invz + kf.cy
            e = _tri_epipole(ex, ey, f2)
            if e is None:
                continue
            live.append(j)
            frames.append(f2)
            F.append(F12)
            epi.append(e)
        res = {}
        if live:
            off = np.zeros(len(frames) + 1, np.int64)
            np.cumsum([len(f.desc) for f in frames], out=off[1:])
            fv_off = np.zeros(len(frames) + 1, np.int64)
            np.cumsum([len(f.fv_node) for f in frames], out=fv_off[1:])
            lvl_off = np.zeros(len(frames) + 1, np.int64)
            np.cumsum([len(f.thr_epi) for f in frames], out=lvl_off[1:])
            cat = lambda k, dt: np.ascontiguousarray(np.concatenate([getattr(f, k) for f in frames]), dt)  # noqa: E731
            fv_idx = np.zeros(int(off[-1]), np.int32)
            for k, f in enumerate(frames):
                fv_idx[off[k]:off[k] + len(f.fv_idx)] = f.fv_idx
            r = tri_match_arrays(cat("desc", np.uint8).reshape(-1, 32), cat("angle", np.float32), cat("xy", np.float64),
                                 cat("octave", np.int32), cat("flags", np.uint8), off, fv_off, cat("fv_node", np.int32),
                                 cat("fv_end", np.int32), fv_idx, lvl_off, cat("thr_epi", np.float64),
                                 cat("thr_ex", np.float64), [(0, k + 1) for k in range(len(live))], np.stack(F),
                                 np.array(epi, np.float64), TH_LOW, bool(bOnlyStereo))
            n1 = len(f1.desc)
            for k, j in enumerate(live):
                if r["stopped"][k]:
                    res[j] = None
                elif not r["status"][k]:
                    res[j] = self._tri_reject(r["match12"][k, :n1], r["bin12"][k, :n1], r["hist"][k])
        out = []
        for j, (kf, F12) in enumerate(todo):
            if j not in res:
                out.append(self.search_for_triangulation(pKF1, kf, F12, bOnlyStereo))
            elif res[j] is None:
                raise StopIteration
            else:
                out.append(res[j])
        return out

    def _tri_reject(self, match12, bin12, hist):
        """The rotation rejection and the result list of search_for_triangulation (ORBMatcher.py:679-696) over
        k_tri_match's raw outputs: compute_three_maxima on the histogram, as the reference ranks it on this host."""
        keep = match12 >= 0
        if self.mbCheckOrientation:
            kept = np.zeros(HISTO_LENGTH + 2, bool)
            counts = [range(c) for c in hist[:HISTO_LENGTH].tolist()]
            kept[np.asarray(self.compute_three_maxima(counts, HISTO_LENGTH))] = True
            keep &= kept[bin12]
        i1 = np.flatnonzero(keep)
        return list(zip(i1.tolist(), match12[i1].tolist()))

    def _sim3_side(self, vpMapPoints, already, Rw, tw, sR, t, pKFo, th, K):
        """One direction of search_by_sim3 (ORBMatcher.py:744-783 / 785-825): best index in pKFo per point.
        K = (fx, fy, cx, cy): the reference projects both directions with pKF1's intrinsics."""
        fx, fy, cx, cy = K
        work = []
        for i, pMP in enumerate(vpMapPoints):
            if not pMP or already[i] or pMP.is_bad():
                continue
            p3Dw = pMP.get_world_pos()
            p3Dc = sR @ (Rw @ p3Dw + tw) + t
            if p3Dc[2] < 0.0:
                continue
            invz = 1.0 / p3Dc[2]
            x, y = p3Dc[0] * invz, p3Dc[1] * invz
            u, v = fx * x + cx, fy * y + cy
            if not pKFo.is_in_image(u, v):
                continue
            maxDistance = pMP.get_max_distance_invariance()
            minDistance = pMP.get_min_distance_invariance()
            dist3D = np.linalg.norm(p3Dc)
            if not (minDistance <= dist3D <= maxDistance):
                continue
            lvl = pMP.predict_scale(dist3D, pKFo)
            vIndices = pKFo.get_features_in_area(u, v, th * pKFo.mvScaleFactors[lvl])
            if not vIndices:
                continue
            cands = [idx for idx in vIndices if lvl - 1 <= pKFo.mvKeysUn[idx].octave <= lvl]
            work.append((i, cands, pMP.get_descriptor()))
        best = [-1] * len(vpMapPoints)
        for (i, cands, _), dq in zip(work, self._batched([(w[2], w[1]) for w in work], pKFo.mDescriptors)):
            best_dist, best_idx = np.inf, -1
            for idx, dist in zip(cands, dq.tolist()):
                if dist < best_dist:
                    best_dist, best_idx = dist, idx
            if best_dist <= TH_HIGH:
                best[i] = best_idx
        return best

    def _sim3_host(self, pKF1, pKF2, vpMatches12, s12, R12, t12, th):
        """search_by_sim3 on the host, point by point (only the Hamming distances run on the device): the fallback
        of the public method."""
        R1w, t1w = pKF1.get_rotation(), pKF1.get_translation()
        R2w, t2w = pKF2.get_rotation(), pKF2.get_translation()
        sR12 = s12 * R12
        sR21 = (1.0 / s12) * R12.T
        t21 = -sR21 @ t12
        vpMapPoints1 = pKF1.get_map_point_matches()
        vpMapPoints2 = pKF2.get_map_point_matches()
        N1, N2 = len(vpMapPoints1), len(vpMapPoints2)
        vbAlreadyMatched1 = [False] * N1
        vbAlreadyMatched2 = [False] * N2
        for i, pMP in enumerate(vpMatches12):
            if pMP:
                vbAlreadyMatched1[i] = True
                idx2 = pMP.get_index_in_keyframe(pKF2)
                if 0 <= idx2 < N2:
                    vbAlreadyMatched2[idx2] = True
        K = (pKF1.fx, pKF1.fy, pKF1.cx, pKF1.cy)
        vnMatch1 = self._sim3_side(vpMapPoints1, vbAlreadyMatched1, R1w, t1w, sR21, t21, pKF2, th, K)
        vnMatch2 = self._sim3_side(vpMapPoints2, vbAlreadyMatched2, R2w, t2w, sR12, t12, pKF1, th, K)
        n_found = 0
        for i1, idx2 in enumerate(vnMatch1):
            if idx2 >= 0 and vnMatch2[idx2] == i1:
                vpMatches12[i1] = vpMapPoints2[idx2]
                n_found += 1
        return n_found, vpMatches12

    def _sim3_one(self, pMP, Rw, tw, sR, t, pKFo, th, K):
        """The best index in pKFo of one point, or -1, with the reference's own expressions on the objects
        (ORBMatcher.py:746-789 / 795-838): _sim3_side for a single item; the few distances are host popcounts."""
        fx, fy, cx, cy = K
        with np.errstate(all="ignore"):
            p3Dw = pMP.get_world_pos()
            p3Dc = sR @ (Rw @ p3Dw + tw) + t
            if p3Dc[2] < 0.0:
                return -1
            invz = 1.0 / p3Dc[2]
            x, y = p3Dc[0] * invz, p3Dc[1] * invz
            u, v = fx * x + cx, fy * y + cy
            if not pKFo.is_in_image(u, v):
                return -1
            maxDistance = pMP.get_max_distance_invariance()
            minDistance = pMP.get_min_distance_invariance()
            dist3D = np.linalg.norm(p3Dc)
            if not (minDistance <= dist3D <= maxDistance):
                return -1
            lvl = pMP.predict_scale(dist3D, pKFo)
            vIndices = pKFo.get_features_in_area(u, v, th * pKFo.mvScaleFactors[lvl])
        d = pMP.get_descriptor()
        best_dist, best_idx = np.inf, -1
        for idx in vIndices:
            if not lvl - 1 <= pKFo.mvKeysUn[idx].octave <= lvl:
                continue
            dist = descriptor_distance(d, pKFo.mDescriptors[idx])
            if dist < best_dist:
                best_dist, best_idx = dist, idx
        return best_idx if best_dist <= TH_HIGH else -1

    @staticmethod
    def _sim3_prep(N1, pKF2, vpMatches12, s12, R12, t12):
        """What one pair adds to a k_sim3_search launch, or None when the arrays cannot express it (the pair then
        takes _sim3_host): (_FuseFrame of pKF2, its map point list, (sR12, t12, sR21, t21) as the reference's
        expressions give them, the same widened exactly as lists, whether any of them is float32)."""
        if not (type(s12) in _TH_SET and np.isfinite(s12) and s12 != 0):
            return None
        if _pose_part(R12, (3, 3)) is None or _pose_part(t12, (3, 1)) is None:
            return None
        if not (isinstance(vpMatches12, list) and len(vpMatches12) == N1):
            return None
        f2 = _fuse_frame(pKF2)
        if f2 is None:
            return None
        vp2 = pKF2.get_map_point_matches()
        if len(vp2) != len(f2.xy):
            return None
        with np.errstate(all="ignore"):
            sR12 = s12 * R12
            sR21 = (1.0 / s12) * R12.T
            t21 = -sR21 @ t12
        sim3 = (sR12, t12, sR21, t21)
        wide = [_pose_part(a, shape) for a, shape in zip(sim3, ((3, 3), (3, 1), (3, 3), (3, 1)))]
        if any(w is None for w in wide):
            return None
        return f2, vp2, sim3, [w[0] for w in wide], any(w[1] for w in wide)

    def _sim3_pairs(self, pKF1, pairs, th):
        """search_by_sim3 of pKF1 with every (pKF2, vpMatches12, s12, R12, t12) of pairs from one k_sim3_search
        launch of two searches per pair: per pair (n_found, vpMatches12), or None for a pair the arrays cannot
        express (nothing of it was touched).  pKF1 is packed once and its live points are sent once; direction 1 of
        a pair indexes them without that pair's already matched ones.  The two directions read nothing the call
        writes, so the results are applied after the launch without an ordered replay."""
        none = [None] * len(pairs)
        if not (type(th) in _TH_SET and np.isfinite(th)):
            return none
        f1 = _fuse_frame(pKF1)
        if f1 is None:
            return none
        vp1 = pKF1.get_map_point_matches()
        N1 = len(vp1)
        if N1 != len(f1.xy):
            return none
        preps = [self._sim3_prep(N1, *pr) for pr in pairs]
        if all(p is None for p in preps):
            return none
        R1w, t1w = pKF1.get_rotation(), pKF1.get_translation()
        K = (pKF1.fx, pKF1.fy, pKF1.cx, pKF1.cy)
        skip = lambda p: not p or p.is_bad()  # noqa: E731
        slot1, rows, descs, f32 = self._search_points(vp1, skip)
        slot1 = np.array(slot1, np.int64)
        f32 = f32 or f1.f32
        frames, kf_at = [f1], {id(pKF1): 0}
        srch_f64, srch_kf, srch_off, item_pt, work = [], [], [0], [], []
        K1 = f1.f64[0:4].tolist()
        for pr, pp in zip(pairs, preps):
            if pp is None:
                continue
            pKF2, vpMatches12 = pr[0], pr[1]
            f2, vp2, sim3, wide, s32 = pp
            f32 = f32 or f2.f32 or s32
            N2 = len(vp2)
            already1, already2 = np.zeros(N1, bool), [False] * N2
            for i, pMP in enumerate(vpMatches12):
                if pMP:
                    already1[i] = True
                    idx2 = pMP.get_index_in_keyframe(pKF2)
                    if 0 <= idx2 < N2:
                        already2[idx2] = True
            it1 = np.flatnonzero((slot1 >= 0) & ~already1)
            alone1 = np.flatnonzero((slot1 == -1) & ~already1)
            slot2, rows2, descs2, p32 = self._search_points([None if a else p for p, a in zip(vp2, already2)], skip)
            slot2 = np.array(slot2, np.int64)
            it2, alone2 = np.flatnonzero(slot2 >= 0), np.flatnonzero(slot2 == -1)
            f32 = f32 or p32
            if id(pKF2) not in kf_at:
                kf_at[id(pKF2)] = len(frames)
                frames.append(f2)
            # direction 1 looks into pKF2 through (R1w, t1w) and (sR21, t21), direction 2 into pKF1 through
            # (R2w, t2w) and (sR12, t12); both project with pKF1's intrinsics
            srch_f64.append(K1 + f1.f64[5:17].tolist() + wide[2] + wide[3])
            srch_f64.append(K1 + f2.f64[5:17].tolist() + wide[0] + wide[1])
            srch_kf += [kf_at[id(pKF2)], 0]
            item_pt += [slot1[it1], slot2[it2] + len(rows)]
            srch_off += [srch_off[-1] + len(it1), srch_off[-1] + len(it1) + len(it2)]
            rows += rows2
            descs += descs2
            work.append((pKF2, vpMatches12, vp2, sim3, it1, alone1, it2, alone2))
        if srch_off[-1]:
            res = self._search_launch(frames, rows, descs, th, f32, sim3=(
                np.array(srch_f64, np.float64), np.array(srch_kf, np.int32), np.array(srch_off, np.int64),
                np.concatenate(item_pt).astype(np.int32)))
            bi, bd, st = res["best_idx"], res["best_dist"], res["status"]
        out, results, s = [], iter(work), 0
        for pp in preps:
            if pp is None:
                out.append(None)
                continue
            pKF2, vpMatches12, vp2, (sR12, t12, sR21, t21), it1, alone1, it2, alone2 = next(results)
            R2w, t2w = pKF2.get_rotation(), pKF2.get_translation()
            sides = []
            for items, alone, vp, pose, pKFo in ((it1, alone1, vp1, (R1w, t1w, sR21, t21), pKF2),
                                                 (it2, alone2, vp2, (R2w, t2w, sR12, t12), pKF1)):
                best = np.full(len(vp), -1, np.int64)
                redo = alone
                if len(items):
                    seg = slice(srch_off[s], srch_off[s + 1])
                    b, d, m = bi[seg], bd[seg], st[seg] != 0
                    ok = ~m & (d >= 0) & (d <= TH_HIGH)
                    best[items[ok]] = b[ok]
                    redo = np.concatenate([alone, items[m]])
                for i in redo.tolist():
                    best[i] = self._sim3_one(vp[i], *pose, pKFo, th, K)
                sides.append(best.tolist())
                s += 1
            vnMatch1, vnMatch2 = sides
            n_found = 0
            for i1, idx2 in enumerate(vnMatch1):
                if idx2 >= 0 and vnMatch2[idx2] == i1:
                    vpMatches12[i1] = vp2[idx2]
                    n_found += 1
            out.append((n_found, vpMatches12))
        return out

    # ORBMatcher.py:713-848
    def search_by_sim3(self, pKF1, pKF2, vpMatches12, s12, R12, t12, th):
        """LoopClosing.compute_sim3's mutual search (LoopClosing.py:203) from one k_sim3_search launch of two
        searches: pKF1's map points into pKF2 through (R1w, t1w) and (sR21, t21), and pKF2's into pKF1 through
        (R2w, t2w) and (sR12, t12), with sR12, sR21 and t21 from the reference's expressions on the host.  The
        prefilter (not pMP or already matched or pMP.is_bad()) and the already-matched flags are taken once on the
        host and only surviving points are sent.  An item that came back ORBFE_FUSE_MARGINAL, or whose point the
        arrays cannot express, is redone alone with the reference's expressions (_sim3_one); otherwise the device's
        candidate counts when best_dist <= TH_HIGH.  The mutual check and the writes into vpMatches12 follow on the
        host in list order.  Neither direction reads what the call writes, so nothing is replayed in order.  The
        host body (_sim3_host) runs instead when _fuse_frame refuses either keyframe (or a keyframe does not have
        one map point slot per feature), when R12 / t12 is not a finite (3, 3) / (3, 1) float32 / float64 array,
        when s12 is not a plain finite non-zero number or the Sim3 parts it gives are not finite, when th is not a
        plain finite number, or when vpMatches12 is not a list with one entry per map point slot of pKF1.  It also
        runs where the HIP runtime sees no device, as for search_by_projection_ckf_scw_mp."""
        if _lib.device_present():
            r = self._sim3_pairs(pKF1, [(pKF2, vpMatches12, s12, R12, t12)], th)[0]
            if r is not None:
                return r
        return self._sim3_host(pKF1, pKF2, vpMatches12, s12, R12, t12, th)

    def search_by_sim3_many(self, pKF1, kfs2, vpMatches12s, s12s, R12s, t12s, th):
        """What this list holds, list for list, from one k_sim3_search launch of two searches per candidate:

            [self.search_by_sim3(pKF1, kf, v, s, R, t, th)
             for kf, v, s, R, t in zip(kfs2, vpMatches12s, s12s, R12s, t12s)]

        pKF1 is packed once and its live map points are sent once for all candidates.  A candidate whose keyframe
        or Sim3 the arrays cannot express (see search_by_sim3) takes the single call at its place.  The loop itself
        runs when two candidates share one vpMatches12 list object (the second would read what the first wrote) and
        where the HIP runtime sees no device."""
        cols = [list(c) for c in (kfs2, vpMatches12s, s12s, R12s, t12s)]
        pairs = list(zip(*cols))
        if any(len(c) != len(pairs) for c in cols):
            raise ValueError("one vpMatches12, s12, R12 and t12 per keyframe")
        res = [None] * len(pairs)
        if _lib.device_present() and len({id(pr[1]) for pr in pairs}) == len(pairs):
            res = self._sim3_pairs(pKF1, pairs, th)
        return [self.search_by_sim3(pKF1, *pr, th) if r is None else r for pr, r in zip(pairs, res)]

    @staticmethod
    def _ckf_pose(Scw):
        """ORBMatcher.py:853-857."""
        sRcw = Scw[:3, :3]
        scw = np.linalg.norm(sRcw[0])
        Rcw = sRcw / scw
        tcw = Scw[:3, 3:4] / scw
        return Rcw, tcw, -Rcw.T @ tcw

    # ORBMatcher.py:850-922
    def search_by_projection_ckf_scw_mp(self, pKF, Scw, vpPoints, vpMatched, th):
        """LoopClosing.compute_sim3's search (LoopClosing.py:234) from one k_scw_search launch: the prefilter in list
        order (pMP.is_bad() or pMP in spAlreadyFound, with spAlreadyFound = set(vpMatched) - {None} taken once),
        blocked[idx] = vpMatched[idx] is not None taken once, then the replay in list order.  An item that came back
        ORBFE_FUSE_MARGINAL, or whose point the arrays cannot express, or whose best candidate an earlier point of
        this call has taken meanwhile, is redone alone against the current vpMatched (_scw_one); otherwise the
        device's candidate is assigned when best_dist <= TH_LOW.  Taking candidates away never changes which of the
        remaining ones is best, so the device's answer stands whenever its candidate is still free.  The host body
        (_ckf_host) runs instead when _fuse_frame refuses the keyframe, when Scw is not a finite 4 x 4 float32 /
        float64 array with a non-zero first row, when th is not a plain finite number, or when vpMatched is not a
        list with one entry per feature.  It also runs where the HIP runtime sees no device: its only device work is
        _batched, the seam the host-logic tests replace, so those tests keep reading the host body."""
        sf = None
        if type(th) in _TH_SET and np.isfinite(th) and isinstance(vpMatched, list) and _lib.device_present():
            sf = self._scw_frame(pKF, Scw, self._ckf_pose)
            if sf is not None and len(vpMatched) != len(sf[0].xy):
                sf = None
        if sf is None:
            return self._ckf_host(pKF, Scw, vpPoints, vpMatched, th)
        f, (Rcw, tcw, Ow) = sf
        if not isinstance(vpPoints, (list, tuple)):
            vpPoints = list(vpPoints)
        spAlreadyFound = set(vpMatched) - {None}
        blocked = np.fromiter((m is not None for m in vpMatched), np.uint8, count=len(vpMatched))
        slot, rows, descs, f32 = self._search_points(vpPoints, lambda p: p.is_bad() or p in spAlreadyFound)
        slot_arr = np.array(slot, np.int64)
        todo = np.flatnonzero(slot_arr == -1)
        if rows:
            res = self._search_launch([f], rows, descs, th, f32 or f.f32, blocked=blocked)
            bi, bd, st = res["best_idx"][0], res["best_dist"][0], res["status"][0]
            # what is left of a point's candidates is never closer than its best: above TH_LOW nothing is assigned
            sent = np.flatnonzero(slot_arr >= 0)
            todo = np.sort(np.concatenate([todo, sent[(st != 0) | ((bi >= 0) & (bd <= TH_LOW))]]))
            bi, bd, st = bi.tolist(), bd.tolist(), st.tolist()
        n_matches = 0
        for i in todo.tolist():
            pMP = vpPoints[i]
            s = slot[i]
            if s >= 0 and not st[s] and vpMatched[bi[s]] is None:
                best_dist, best_idx = bd[s], bi[s]
            else:
                best_dist, best_idx = self._scw_one(pKF, pMP, Rcw, tcw, Ow, th, vpMatched)
            if best_idx >= 0 and best_dist <= TH_LOW:
                vpMatched[best_idx] = pMP
                n_matches += 1
        return n_matches, vpMatched

    def _ckf_host(self, pKF, Scw, vpPoints, vpMatched, th):
        """search_by_projection_ckf_scw_mp on the host, point by point (only the Hamming distances run on the
        device): the fallback of the public method."""
        sRcw = Scw[:3, :3]
        scw = np.linalg.norm(sRcw[0])
        Rcw = sRcw / scw
        tcw = Scw[:3, 3:4] / scw
        Ow = -Rcw.T @ tcw
        spAlreadyFound = set(vpMatched) - {None}
        work = []
        for pMP in vpPoints:
            if pMP.is_bad() or pMP in spAlreadyFound:
                continue
            pr = self._project_checked(pMP, pKF, Rcw, tcw, True)
            if pr is None:
                continue
            u, v, _, p3Dw = pr
            if not pKF.is_in_image(u, v):
                continue
            lvl = self._distance_gates(pMP, pKF, p3Dw, Ow)
            if lvl is None:
                continue
            vIndices = pKF.get_features_in_area(u, v, th * pKF.mvScaleFactors[lvl])
            if not vIndices:
                continue
            cands = [i for i in vIndices if lvl - 1 <= pKF.mvKeysUn[i].octave <= lvl]
            work.append((pMP, cands, pMP.get_descriptor()))
        n_matches = 0
        for (pMP, cands, _), dq in zip(work, self._batched([(w[2], w[1]) for w in work], pKF.mDescriptors)):
            best_dist, best_idx = 256, -1
            for idx, dist in zip(cands, dq.tolist()):
                if vpMatched[idx] is not None:
                    continue
                if dist < best_dist:
                    best_dist = dist
                    best_idx = idx
            if best_dist <= TH_LOW:
                vpMatched[best_idx] = pMP
                n_matches += 1
        return n_matches, vpMatched

    @staticmethod
    def _fkf_job(CurrentFrame, th, ORBdist):
        """_fkf_frame(CurrentFrame) when one search of search_by_projection_f_kf_f can run on the device, else
        None: see the conditions there."""
        if not (type(th) in _TH_SET and np.isfinite(th) and type(ORBdist) in (int, float) and ORBdist < 256):
            return None
        f = _fkf_frame(CurrentFrame)
        if f is None:
            return None
        mvp = CurrentFrame.mvpMapPoints
        if not (isinstance(mvp, list) and len(mvp) == len(f.xy) == CurrentFrame.N):
            return None
        return f

    def _fkf_one(self, CurrentFrame, pMP, Rcw, tcw, Ow, th):
        """(bestDist, bestIdx2) of one point against the current CurrentFrame.mvpMapPoints with the reference's own
        expressions on the objects (ORBMatcher.py:939-983), raising what they raise; the few distances are host
        popcounts."""
        with np.errstate(all="ignore"):
            x3Dw = pMP.get_world_pos()
            x3Dc = np.dot(Rcw, x3Dw) + tcw
            xc = x3Dc[0]
            yc = x3Dc[1]
            invzc = 1.0 / x3Dc[2]
            u = CurrentFrame.fx * xc * invzc + CurrentFrame.cx
            v = CurrentFrame.fy * yc * invzc + CurrentFrame.cy
            if u < CurrentFrame.mnMinX or u > CurrentFrame.mnMaxX or v < CurrentFrame.mnMinY or v > CurrentFrame.mnMaxY:
                return 256, -1
            PO = x3Dw - Ow
            dist3D = np.linalg.norm(PO)
            maxDistance = pMP.get_max_distance_invariance()
            minDistance = pMP.get_min_distance_invariance()
            if dist3D < minDistance or dist3D > maxDistance:
                return 256, -1
            lvl = pMP.predict_scale(dist3D, CurrentFrame)
            vIndices2 = CurrentFrame.get_features_in_area(u, v, th * CurrentFrame.mvScaleFactors[lvl], lvl - 1, lvl + 1)
        best_dist, best_idx2 = 256, -1
        if not vIndices2:
            return best_dist, best_idx2
        dMP = pMP.get_descriptor()
        for i2 in vIndices2:
            if CurrentFrame.mvpMapPoints[i2]:
                continue
            dist = descriptor_distance(dMP, CurrentFrame.mDescriptors[i2])
            if dist < best_dist:
                best_dist = dist
                best_idx2 = i2
        return best_dist, best_idx2

    def _fkf_jobs(self, jobs, th, ORBdist):
        """search_by_projection_f_kf_f for every (CurrentFrame, pKF, sAlreadyFound, _fkf_frame(CurrentFrame)) of
        jobs, whose frames are distinct objects with distinct mvpMapPoints lists, from one k_fkf_search launch of
        one search per job: the match counts.  Per job in the reference's order: the prefilter in list order, the
        blocked bytes (the truth value of every mvpMapPoints slot) taken once, then after the launch the replay in
        list order (see search_by_projection_f_kf_f)."""
        frames, rows, descs, f32, preps = [], [], [], False, []
        srch_off, item_pt, blocked = [0], [], []
        for CurrentFrame, pKF, sAlreadyFound, f in jobs:
            vpMPs = pKF.get_map_point_matches()
            slot, rows_j, descs_j, p32 = self._search_points(
                vpMPs, lambda p: not (p and not p.is_bad() and p not in sAlreadyFound), normal=False)
            slot = np.array(slot, np.int64).reshape(-1)
            sent = np.flatnonzero(slot >= 0)
            item_pt.append(slot[sent] + len(rows))
            srch_off.append(srch_off[-1] + len(sent))
            rows += rows_j
            descs += descs_j
            f32 = f32 or p32 or f.f32
            mvp = CurrentFrame.mvpMapPoints
            blocked.append(np.fromiter((bool(m) for m in mvp), np.uint8, count=len(mvp)))
            frames.append(f)
            preps.append((vpMPs, slot, sent))
        if srch_off[-1]:
            res = self._search_launch(frames, rows, descs, th, f32, blocked=np.concatenate(blocked), fkf=(
                np.arange(len(jobs), dtype=np.int32), np.array(srch_off, np.int64),
                np.concatenate(item_pt).astype(np.int32)))
            bi_all, bd_all, st_all = res["best_idx"], res["best_dist"], res["status"]
        out = []
        factor = 1.0 / HISTO_LENGTH
        for q, ((CurrentFrame, pKF, _, f), (vpMPs, slot, sent)) in enumerate(zip(jobs, preps)):
            Rcw, tcw, Ow = f.pose
            mvp = CurrentFrame.mvpMapPoints
            rot_hist = [[] for _ in range(HISTO_LENGTH)]
            todo = np.flatnonzero(slot == -1)
            at = {}
            if len(sent):
                seg = slice(srch_off[q], srch_off[q + 1])
                bi, bd, st = bi_all[seg], bd_all[seg], st_all[seg]
                # what is left of a point's candidates is never closer than its best: an unmarked item above
                # ORBdist, or without a candidate, assigns nothing whatever was taken meanwhile
                live = (st != 0) | ((bi >= 0) & (bd <= ORBdist))
                todo = np.sort(np.concatenate([todo, sent[live]]))
                at = dict(zip(sent[live].tolist(), zip(bi[live].tolist(), bd[live].tolist(), st[live].tolist())))
            n_matches = 0
            for i in todo.tolist():
                pMP = vpMPs[i]
                dev = at.get(i)
                if dev is not None and not dev[2] and not mvp[dev[0]]:
                    best_idx2, best_dist = dev[0], dev[1]
                else:
                    best_dist, best_idx2 = self._fkf_one(CurrentFrame, pMP, Rcw, tcw, Ow, th)
                if best_dist <= ORBdist:
                    mvp[best_idx2] = pMP
                    n_matches += 1
                    if self.mbCheckOrientation:
                        rot = pKF.mvKeysUn[i].angle - CurrentFrame.mvKeysUn[best_idx2].angle
                        if rot < 0.0:
                            rot += 360.0
                        b = round(rot * factor)
                        if b == HISTO_LENGTH:
                            b = 0
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(best_idx2)
            if self.mbCheckOrientation:
                n_matches -= self._reject_by_rotation(rot_hist, lambda i, mvp=mvp: mvp.__setitem__(i, None))
            out.append(n_matches)
        return out

    # ORBMatcher.py:924-1008
    def search_by_projection_f_kf_f(self, CurrentFrame, pKF, sAlreadyFound, th, ORBdist):
        """Tracking.relocalization's search (Tracking.py:661-763) from one k_fkf_search launch: the prefilter in list
        order (pMP and not pMP.is_bad() and pMP not in sAlreadyFound), blocked[i] = bool(mvpMapPoints[i]) taken once,
        then the replay in list order.  An item that came back ORBFE_FUSE_MARGINAL, or whose point the arrays cannot
        express, or whose best feature an earlier item of this call has taken meanwhile, is redone alone against the
        current mvpMapPoints with the reference's expressions (_fkf_one, raising what they raise); otherwise the
        device's answer stands and is assigned when best_dist <= ORBdist.  Taking candidates away never makes a
        remaining one closer, so an unmarked item above ORBdist needs no redo.  The rotation histogram and its
        rejection follow as in the reference.  The host body (_fkf_host) runs instead when the HIP runtime sees no
        device (its only device work is _batched, the seam the host-logic tests replace), when th is not a plain
        finite number, when ORBdist is not a plain int / float below 256 (from 256 on the reference assigns to index
        -1 once every candidate is taken), when CurrentFrame.mvpMapPoints is not a list of N entries, or when
        _fkf_frame refuses the frame."""
        if _lib.device_present():
            f = self._fkf_job(CurrentFrame, th, ORBdist)
            if f is not None:
                return self._fkf_jobs([(CurrentFrame, pKF, sAlreadyFound, f)], th, ORBdist)[0]
        return self._fkf_host(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)

    def search_by_projection_f_kf_f_many(self, frames, kfs, sAlreadyFounds, th, ORBdist):
        """What this list holds, value for value and leaving every frame's mvpMapPoints as the loop leaves it, from
        one k_fkf_search launch of one search per frame:

            [self.search_by_projection_f_kf_f(f, kf, s, th, ORBdist)
             for f, kf, s in zip(frames, kfs, sAlreadyFounds)]

        (several lost frames relocalising at once, or one frame against several keyframes after a host-side copy
        of it per keyframe).  Each frame is packed once.  A frame that cannot take the device path (see
        search_by_projection_f_kf_f) takes the single call at its place.  The loop itself runs when a frame object,
        or an mvpMapPoints list, occurs twice (its second search would read what the first assigned) and where the
        HIP runtime sees no device."""
        cols = [list(c) for c in (frames, kfs, sAlreadyFounds)]
        jobs = list(zip(*cols))
        if any(len(c) != len(jobs) for c in cols):
            raise ValueError("one keyframe and one sAlreadyFound per frame")
        res = [None] * len(jobs)
        distinct = len({id(j[0]) for j in jobs}) == len(jobs) == len({id(getattr(j[0], "mvpMapPoints", j[0]))
                                                                     for j in jobs})
        if jobs and distinct and _lib.device_present():
            packed = [self._fkf_job(j[0], th, ORBdist) for j in jobs]
            take = [k for k, f in enumerate(packed) if f is not None]
            if take:
                for k, n in zip(take, self._fkf_jobs([jobs[k] + (packed[k],) for k in take], th, ORBdist)):
                    res[k] = n
        return [self.search_by_projection_f_kf_f(*j, th, ORBdist) if r is None else r for j, r in zip(jobs, res)]

    # Tracking.py:439-468
    def _local_job(self, frame, th, viewing_cos_limit):
        """_local_frame(frame) when one search_local_points can run on the device, else None: see the conditions
        there."""
        if type(self).radius_by_viewing_cos is not ORBMatcher.radius_by_viewing_cos:
            return None
        if not (type(th) in _TH_SET and np.isfinite(th) and type(viewing_cos_limit) in _TH_SET
                and np.isfinite(viewing_cos_limit)):
            return None
        f = _local_frame(frame)
        if f is None:
            return None
        mvp = frame.mvpMapPoints
        if not (isinstance(mvp, list) and len(mvp) == len(f.xy) == frame.N):
            return None
        return f

    def _local_loop(self, frame, vpMapPoints, th, viewing_cos_limit):
        """Tracking.search_local_points' loop with the frame's own is_in_frustum and search_by_projection_f_p: the
        fallback of search_local_points."""
        nToMatch = 0
        for pMP in vpMapPoints:
            if pMP.mnLastFrameSeen == frame.mnId:
                continue
            if pMP.is_bad():
                continue
            if frame.is_in_frustum(pMP, viewing_cos_limit):
                pMP.increase_visible()
                nToMatch += 1
        return nToMatch, (self.search_by_projection_f_p(frame, vpMapPoints, th) if nToMatch > 0 else None)

    def _fp_one(self, frame, pMP, th):
        """The body of search_by_projection_f_p's loop (ORBMatcher.py:226-281) for one point that is tracked in view
        and not bad, with the reference's expressions on the objects against the current frame.mvpMapPoints, raising
        what they raise; the few distances are host popcounts.  True when the point was assigned."""
        b_factor = th != 1.0
        n_predicted_level = pMP.mnTrackScaleLevel
        r = self.radius_by_viewing_cos(pMP.mTrackViewCos)
        if b_factor:
            r *= th
        v_indices = frame.get_features_in_area(pMP.mTrackProjX, pMP.mTrackProjY,
                                               r * frame.mvScaleFactors[n_predicted_level], n_predicted_level - 1,
                                               n_predicted_level)
        if not v_indices:
            return False
        MPdescriptor = pMP.get_descriptor()
        best_dist = 256
        best_level = -1
        best_dist2 = 256
        best_level2 = -1
        best_idx = -1
        for idx in v_indices:
            if frame.mvpMapPoints[idx]:
                if frame.mvpMapPoints[idx].observations() > 0:
                    continue
            if frame.mvuRight[idx] > 0:
                er = abs(pMP.mTrackProjXR - frame.mvuRight[idx])
                if er > r * frame.mvScaleFactors[n_predicted_level]:
                    continue
            dist = descriptor_distance(MPdescriptor, frame.mDescriptors[idx])
            if dist < best_dist:
                best_dist2 = best_dist
                best_dist = dist
                best_level2 = best_level
                best_level = frame.mvKeysUn[idx].octave
                best_idx = idx
            elif dist < best_dist2:
                best_level2 = frame.mvKeysUn[idx].octave
                best_dist2 = dist
        if best_dist <= TH_HIGH:
            if best_level == best_level2 and best_dist > self.mfNNratio * best_dist2:
                return False
            frame.mvpMapPoints[best_idx] = pMP
            return True
        return False

    @classmethod
    def _local_points(cls, vp, mn_id):
        """_search_points for search_local_points, whose lists are long and run on every frame: the loop's two skips
        in list order, then the kept points' positions, normals, distances and descriptors gathered by C-level map()
        and stacked once where they are uniform (arrays of one shape and dtype each, distances of _DIST_SET); a row
        that is not finite is a point the arrays cannot express.  Anything else takes _search_points point by point.
        Returns (slot per list position, (m, 9) rows, (m, 32) descriptors, any float32)."""
        skip = [p.mnLastFrameSeen == mn_id or p.is_bad() for p in vp]
        kept = list(compress(vp, map(operator.not_, skip)))
        m = len(kept)
        pos, nrm = list(map(_WORLD_POS, kept)), list(map(operator.methodcaller("get_normal"), kept))
        d3 = (list(map(operator.methodcaller("get_min_distance_invariance"), kept)),
              list(map(operator.methodcaller("get_max_distance_invariance"), kept)),
              list(map(operator.attrgetter("mfMaxDistance"), kept)))
        descs = list(map(_DESCRIPTOR, kept))

        def uniform(arrs, shapes, dts):
            return (set(map(type, arrs)) == _NDARRAY_SET and len(set(map(_SHAPE, arrs))) == 1
                    and arrs[0].shape in shapes and len(set(map(_DTYPE, arrs))) == 1 and arrs[0].dtype in dts)
        if not (m and uniform(pos, ((3, 1),), _POSE_DT) and uniform(nrm, ((3, 1),), _POSE_DT)
                and uniform(descs, ((32,), (1, 32), (32, 1)), (_U8_DT,))
                and all(set(map(type, d)) <= _DIST_SET for d in d3)):
            skipped = iter(skip)
            slot, rows, descs, f32 = cls._search_points(vp, lambda p: next(skipped), f32_dist=True)
            return (np.array(slot, np.int64).reshape(-1), np.array(rows, np.float64).reshape(-1, _lib.ORBFE_FUSE_PT_F64),
                    np.array(descs, np.uint8).reshape(-1, 32), f32)
        rows = np.empty((m, _lib.ORBFE_FUSE_PT_F64), np.float64)
        rows[:, 0:3] = np.concatenate(pos).reshape(m, 3)
        rows[:, 3:6] = np.concatenate(nrm).reshape(m, 3)
        for c, d in enumerate(d3):
            rows[:, 6 + c] = d
        ok = np.isfinite(rows).all(axis=1)
        slot = np.full(len(vp), -2, np.int64)
        at = np.flatnonzero(~np.array(skip, bool))
        slot[at] = np.where(ok, np.cumsum(ok) - 1, -1)
        return (slot, rows[ok], np.concatenate(descs).reshape(m, 32)[ok],
                pos[0].dtype == _F32_DT or nrm[0].dtype == _F32_DT)

    def _local_jobs(self, jobs, th, viewing_cos_limit):
        """search_local_points for every (frame, vpMapPoints, _local_frame(frame)) of jobs, whose frames are distinct
        objects with distinct mvpMapPoints lists, from one k_local_search launch of one search per job: the
        (nToMatch, n_matches) pairs.  Per job in the reference's order: the loop's two skips in list order, the
        blocked bytes (a slot holding a point with observations) taken once, then after the launch the frustum
        half and the replay, frame by frame (see search_local_points)."""
        from .frame import is_in_frustum_many
        frames, rows, descs, f32, preps, n_rows = [], [], [], False, [], 0
        srch_off, item_pt, blocked = [0], [], []
        for frame, vp, f in jobs:
            slot, rows_j, descs_j, p32 = self._local_points(vp, frame.mnId)
            sent = np.flatnonzero(slot >= 0)
            item_pt.append(slot[sent] + n_rows)
            srch_off.append(srch_off[-1] + len(sent))
            n_rows += len(rows_j)
            rows.append(rows_j)
            descs.append(descs_j)
            f32 = f32 or p32 or f.f32
            blocked.append(_blocked(frame))
            frames.append(f)
            preps.append((slot, sent))
        if srch_off[-1]:
            res = self._search_launch(frames, np.concatenate(rows), np.concatenate(descs), th, f32,
                                      blocked=np.concatenate(blocked), local=(
                np.full(len(jobs), float(viewing_cos_limit)), np.arange(len(jobs), dtype=np.int32),
                np.array(srch_off, np.int64), np.concatenate(item_pt).astype(np.int32), th != 1.0))
        out = []
        nnratio = self.mfNNratio
        for q, ((frame, vp, f), (slot, sent)) in enumerate(zip(jobs, preps)):
            # the frustum half: what an unmarked item decided stands; the attributes, and the decision of a marked
            # item or of a point the arrays cannot express, come from the reference's expressions on the host
            dev = {}
            if len(sent):
                seg = slice(srch_off[q], srch_off[q + 1])
                st, view = res["status"][seg], res["in_view"][seg]
                for i in sent[(st == 0) & (view == 0)].tolist():
                    vp[i].mbTrackInView = False
                live = (st != 0) | (view != 0)
                dev = dict(zip(sent[live].tolist(), zip(
                    st[live].tolist(), res["level"][seg][live].tolist(), res["best_idx"][seg][live].tolist(),
                    res["best_dist"][seg][live].tolist(), res["second_idx"][seg][live].tolist(),
                    res["second_dist"][seg][live].tolist())))
            host = sorted(list(dev) + np.flatnonzero(slot == -1).tolist())
            seen = dict(zip(host, is_in_frustum_many(frame, [vp[i] for i in host], viewing_cos_limit)))
            nToMatch = 0
            for i in host:
                if seen[i]:
                    vp[i].increase_visible()
                    nToMatch += 1
            if nToMatch == 0:
                out.append((0, None))
                continue
            # the replay of search_by_projection_f_p, in list order
            mvp, kps = frame.mvpMapPoints, frame.mvKeysUn
            n_matches = 0
            for i in sorted(np.flatnonzero(slot == -2).tolist() + [i for i in host if seen[i]]):
                pMP = vp[i]
                d = dev.get(i)
                if slot[i] == -2:
                    # skipped by the loop above: searched where it is still tracked in view from an earlier frame
                    if not pMP.mbTrackInView or pMP.is_bad():
                        continue
                    d = None
                if d is not None and not d[0] and pMP.mnTrackScaleLevel == d[1]:
                    _, _, bi, bd, si, sd = d
                    # what is left of a point's candidates is never closer than its best: an unmarked item above
                    # TH_HIGH, or without a candidate, assigns nothing whatever was taken meanwhile
                    if bi < 0 or bd > TH_HIGH:
                        continue
                    m, m2 = mvp[bi], (mvp[si] if si >= 0 else None)
                    if not ((m and m.observations() > 0) or (m2 and m2.observations() > 0)):
                        # a distance of 256 never enters the reference's second place
                        best_level2, best_dist2 = (kps[si].octave, sd) if si >= 0 and sd < 256 else (-1, 256)
                        if kps[bi].octave == best_level2 and bd > nnratio * best_dist2:
                            continue
                        mvp[bi] = pMP
                        n_matches += 1
                        continue
                if self._fp_one(frame, pMP, th):
                    n_matches += 1
            out.append((nToMatch, n_matches))
        return out

    def search_local_points(self, frame, vpMapPoints, th, viewing_cos_limit=0.5):
        """Tracking.search_local_points (Tracking.py:439-468) from one k_local_search launch: what this gives, return
        values and side effects in the same order,

            nToMatch = 0
            for pMP in vpMapPoints:
                if pMP.mnLastFrameSeen == frame.mnId: continue
                if pMP.is_bad(): continue
                if frame.is_in_frustum(pMP, viewing_cos_limit):
                    pMP.increase_visible(); nToMatch += 1
            n = self.search_by_projection_f_p(frame, vpMapPoints, th) if nToMatch > 0 else None

        as (nToMatch, n).  The points the loop does not skip are packed once and launched, with
        blocked[i] = mvpMapPoints[i] holds a point with observations, taken once.  in_view and level of an item that
        did not come back ORBFE_FUSE_MARGINAL stand; a marked item, and a point the arrays cannot express, is decided
        by the reference's expressions.  Every attribute is_in_frustum writes comes from frame.is_in_frustum_many on
        the host, never from the kernel.  Then the replay in list order: an item's best candidate is assigned when it
        passes TH_HIGH and the ratio test against the second (on the host, with the Python operands); an item is
        redone alone against the current mvpMapPoints with the reference's expressions (_fp_one) when it is marked,
        when its best or second feature has meanwhile been taken by a point with observations, or when the loop
        skipped its point but the point is still tracked in view (it is searched with its stored projections, at its
        place in the list).  Taking candidates away never makes a remaining one closer, so an unmarked item above
        TH_HIGH needs no redo (see search_by_projection_f_kf_f).  The loop itself, with frame.is_in_frustum and
        search_by_projection_f_p, runs instead when the HIP runtime sees no device, when th or the limit is not a
        plain finite number, when radius_by_viewing_cos is overridden, when frame.mvpMapPoints is not a list of N
        entries, or when _local_frame refuses the frame."""
        if _lib.device_present():
            f = self._local_job(frame, th, viewing_cos_limit)
            if f is not None:
                return self._local_jobs([(frame, list(vpMapPoints), f)], th, viewing_cos_limit)[0]
        return self._local_loop(frame, vpMapPoints, th, viewing_cos_limit)

    def search_local_points_many(self, frames, lists, th, viewing_cos_limit=0.5):
        """[self.search_local_points(f, vp, th, viewing_cos_limit) for f, vp in zip(frames, lists)], value for value
        and side effect for side effect, from one k_local_search launch of one search per frame; the frustum halves
        and the replays go frame by frame, in order.  A frame that cannot take the device path takes the single call
        at its place.  The loop itself runs when a frame object, or an mvpMapPoints list, occurs twice (its second
        search would read what the first assigned) and where the HIP runtime sees no device.  A map point may occur
        in several lists: the kernel reads only what no search writes, and each frame's frustum half rewrites the
        point's attributes before that frame's replay, as the loop does."""
        frames, lists = list(frames), [list(vp) for vp in lists]
        if len(frames) != len(lists):
            raise ValueError("one map point list per frame")
        res = [None] * len(frames)
        distinct = len({id(f) for f in frames}) == len(frames) == len({id(getattr(f, "mvpMapPoints", f))
                                                                      for f in frames})
        if frames and distinct and _lib.device_present():
            packed = [self._local_job(f, th, viewing_cos_limit) for f in frames]
            take = [k for k, f in enumerate(packed) if f is not None]
            if take:
                for k, r in zip(take, self._local_jobs([(frames[k], lists[k], packed[k]) for k in take], th,
                                                       viewing_cos_limit)):
                    res[k] = r
        return [self.search_local_points(f, vp, th, viewing_cos_limit) if r is None else r
                for f, vp, r in zip(frames, lists, res)]

    # ORBMatcher.py:291-393
    @staticmethod
    def _ff_job(cur, last, th):
        """What one pair of search_by_projection_f_f_many needs before the launch, or None when the pair takes the
        single call: (_ff_frame(cur), mode, candidates, their octaves).  mode is 1 where the reference's b_forward
        holds, else 2 where its b_backward holds, else 0, from the reference's own expressions."""
        if not (type(th) in _TH_SET and np.isfinite(th)):
            return None
        try:
            Tl, lmps, lout, n_last, keys = last.mTcw, last.mvpMapPoints, last.mvbOutlier, last.N, last.mvKeys
            if not (type(Tl) is np.ndarray and Tl.shape == (4, 4) and Tl.dtype in _POSE_DT
                    and bool(np.isfinite(Tl).all())):
                return None
            f = _ff_frame(cur)
            if f is None:
                return None
            mvp = cur.mvpMapPoints
            if not (isinstance(mvp, list) and len(mvp) == len(f.xy) == cur.N):
                return None
            Rcw, tcw = f.pose[0], f.pose[1]
            with np.errstate(all="ignore"):
                twc = -Rcw.T @ tcw
                Rlw = Tl[:3, :3]
                tlw = Tl[:3, 3:4]
                tlc = Rlw @ twc + tlw
                b_forward = tlc[2] > cur.mb
                b_backward = -tlc[2] > cur.mb
            mode = 1 if b_forward else (2 if b_backward else 0)
            if len(lmps) >= n_last and len(lout) >= n_last:  # the same selection with C-level iteration
                live = list(compress(range(n_last), map(bool, lmps)))
                cand = list(compress(live, map(operator.not_, map(lout.__getitem__, live))))
            else:  # the reference's indexing (and its IndexError)
                cand = [i for i in range(n_last) if lmps[i] and not lout[i]]
            octs = list(map(_OCTAVE, map(keys.__getitem__, cand)))
        except (AttributeError, IndexError, TypeError, ValueError):
            return None
        if not set(map(type, octs)) <= _INT_SET or (octs and not 0 <= min(octs) <= max(octs) < int(f.i32[2])):
            return None
        return f, mode, cand, octs

    def _ff_one(self, cur, last, i, pMP, th, mode, Rcw, tcw):
        """(best_dist, best_idx2) of one point of the last frame against the current cur.mvpMapPoints with the
        reference's own expressions on the objects (ORBMatcher.py:314-367), raising what they raise; the few
        distances are host popcounts."""
        with np.errstate(all="ignore"):
            x3Dw = pMP.get_world_pos()
            x3Dc = Rcw @ x3Dw + tcw
            xc, yc, zc = x3Dc[0][0], x3Dc[1][0], x3Dc[2][0]
            invzc = 1.0 / zc
            if invzc < 0:
                return 256, -1
            u = cur.fx * xc * invzc + cur.cx
            v = cur.fy * yc * invzc + cur.cy
            if u < cur.mnMinX or u > cur.mnMaxX:
                return 256, -1
            if v < cur.mnMinY or v > cur.mnMaxY:
                return 256, -1
            n_last_octave = last.mvKeys[i].octave
            radius = th * cur.mvScaleFactors[n_last_octave]
            if mode == 1:
                v_indices2 = cur.get_features_in_area(u, v, radius, n_last_octave, -1)
            elif mode == 2:
                v_indices2 = cur.get_features_in_area(u, v, radius, 0, n_last_octave)
            else:
                v_indices2 = cur.get_features_in_area(u, v, radius, n_last_octave - 1, n_last_octave + 1)
            best_dist, best_idx2 = 256, -1
            if not v_indices2:
                return best_dist, best_idx2
            dMP = pMP.get_descriptor()
            for i2 in v_indices2:
                if cur.mvpMapPoints[i2]:
                    if cur.mvpMapPoints[i2].observations() > 0:
                        continue
                if cur.mvuRight[i2] > 0:
                    ur = u - cur.mbf * invzc
                    er = abs(ur - cur.mvuRight[i2])
                    if er > radius:
                        continue
                dist = descriptor_distance(dMP, cur.mDescriptors[i2])
                if dist < best_dist:
                    best_dist = dist
                    best_idx2 = i2
        return best_dist, best_idx2

    def _ff_jobs(self, jobs):
        """search_by_projection_f_f for every (cur, last, th, _ff_job(cur, last, th)) of jobs, whose current frames
        are distinct objects with distinct mvpMapPoints lists that no pair reads as its last frame, from one
        k_ff_search launch of one search per job: the match counts.  Per job in the reference's order: the
        candidates in list order, the blocked bytes (a slot holding a point with observations) taken once, then
        after the launch the replay in list order (see search_by_projection_f_f_many)."""
        frames, rows, descs, f32, preps, n_rows = [], [], [], False, [], 0
        srch_off, item_pt, item_level, blocked = [0], [], [], []
        for cur, last, th, (f, mode, cand, octs) in jobs:
            pts = list(map(last.mvpMapPoints.__getitem__, cand))
            pos, dsc = list(map(_WORLD_POS, pts)), list(map(_DESCRIPTOR, pts))
            m = len(pts)
            if (m and set(map(type, pos)) == _NDARRAY_SET and set(map(_SHAPE, pos)) == {(3, 1)}
                    and len(set(map(_DTYPE, pos))) == 1 and pos[0].dtype in _POSE_DT
                    and set(map(type, dsc)) == _NDARRAY_SET and set(map(_DTYPE, dsc)) == {_U8_DT}
                    and set(map(_SIZE, dsc)) == {32} and len(set(map(_SHAPE, dsc))) == 1):
                # uniform points, gathered above by C-level map() and stacked once; a row that is not finite is a
                # point the arrays cannot express
                P = np.concatenate(pos).reshape(m, 3).astype(np.float64)
                sent = np.flatnonzero(np.isfinite(P).all(axis=1))
                rows_j = np.zeros((len(sent), _lib.ORBFE_FUSE_PT_F64), np.float64)
                rows_j[:, 0:3] = P[sent]
                descs_j = np.concatenate(dsc).reshape(m, 32)[sent]
                f32 = f32 or (len(sent) > 0 and pos[0].dtype == _F32_DT)
                sent = sent.tolist()
            else:
                sent, rows_j, descs_j = [], [], []
                for c, (x, d) in enumerate(zip(pos, dsc)):
                    pp = _pose_part(x, (3, 1))
                    if pp is None or not (type(d) is np.ndarray and d.dtype == _U8_DT and d.size == 32):
                        continue  # redone alone
                    sent.append(c)
                    rows_j.append(pp[0] + [0.0] * 6)
                    descs_j.append(d.reshape(32))
                    f32 = f32 or pp[1]
                rows_j = np.array(rows_j, np.float64).reshape(-1, _lib.ORBFE_FUSE_PT_F64)
                descs_j = np.array(descs_j, np.uint8).reshape(-1, 32)
            item_pt.append(np.arange(n_rows, n_rows + len(sent), dtype=np.int32))
            item_level.append(np.array(octs, np.int64)[sent].astype(np.int32))
            n_rows += len(sent)
            rows.append(rows_j)
            descs.append(descs_j)
            srch_off.append(srch_off[-1] + len(sent))
            f32 = f32 or f.f32
            blocked.append(_blocked(cur))
            frames.append(f)
            preps.append(sent)
        if srch_off[-1]:
            res = self._search_launch(frames, np.concatenate(rows), np.concatenate(descs), 0.0, f32,
                                      blocked=np.concatenate(blocked), ff=(
                np.array([float(j[2]) for j in jobs], np.float64), np.array([j[3][1] for j in jobs], np.int32),
                np.arange(len(jobs), dtype=np.int32), np.array(srch_off, np.int64), np.concatenate(item_pt),
                np.concatenate(item_level)))
            bi_all, bd_all, st_all = (res[k].tolist() for k in FF_OUTPUTS)
        out = []
        factor = 1.0 / HISTO_LENGTH
        for q, ((cur, last, th, (f, mode, cand, octs)), sent) in enumerate(zip(jobs, preps)):
            Rcw, tcw = f.pose[0], f.pose[1]
            lmps, mvp = last.mvpMapPoints, cur.mvpMapPoints
            at = dict(zip(sent, range(srch_off[q], srch_off[q + 1])))
            rot_hist = [[] for _ in range(HISTO_LENGTH)]
            n_matches = 0
            for c, i in enumerate(cand):
                pMP = lmps[i]
                j = at.get(c)
                if j is not None and not st_all[j]:
                    # what is left of a point's candidates is never closer than its best: an unmarked item above
                    # TH_HIGH, or without a candidate, assigns nothing whatever was taken meanwhile
                    best_idx2, best_dist = bi_all[j], bd_all[j]
                    if best_idx2 < 0 or best_dist > TH_HIGH:
                        continue
                    m = mvp[best_idx2]
                    if m and m.observations() > 0:
                        best_dist, best_idx2 = self._ff_one(cur, last, i, pMP, th, mode, Rcw, tcw)
                else:
                    best_dist, best_idx2 = self._ff_one(cur, last, i, pMP, th, mode, Rcw, tcw)
                if best_dist <= TH_HIGH:
                    mvp[best_idx2] = pMP
                    n_matches += 1
                    if self.mbCheckOrientation:
                        rot = last.mvKeysUn[i].angle - cur.mvKeysUn[best_idx2].angle
                        if rot < 0.0:
                            rot += 360.0
                        b = round(rot * factor)
                        if b == HISTO_LENGTH:
                            b = 0
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(best_idx2)
            if self.mbCheckOrientation:
                # a feature assigned twice stands twice in the histogram and is counted, and rejected, twice
                ind1, ind2, ind3 = self.compute_three_maxima(rot_hist, HISTO_LENGTH)
                for b in range(HISTO_LENGTH):
                    if b not in (ind1, ind2, ind3):
                        for idx in rot_hist[b]:
                            mvp[idx] = None
                            n_matches -= 1
            out.append(n_matches)
        return out

    def search_by_projection_f_f_many(self, current_frames, last_frames, th):
        """What this list holds, value for value and leaving every current frame's mvpMapPoints as the loop leaves it,
        from one k_ff_search launch of one search per pair:

            [self.search_by_projection_f_f(c, l, th_k) for c, l, th_k in zip(current_frames, last_frames, ths)]

        (several trackers stepped in lockstep running Tracking.track_with_motion_model's search).  th is a plain
        number for all pairs, or a sequence of one per pair (a tracker retries its pair with twice the th).  Per
        pair, before the launch: b_forward / b_backward by the reference's expressions, the candidates i with
        mvpMapPoints[i] and not mvbOutlier[i] in list order, blocked[i2] = the slot holds a point with observations,
        taken once; eps is float32's where the current pose or a sent position is float32.  After the launch the
        replay in list order: the device's answer stands unless the item came back ORBFE_FUSE_MARGINAL, its point
        cannot be expressed as arrays (a position that is not a finite (3, 1) float32 / float64 array, a descriptor
        that is not 32 bytes of uint8), or its best feature has meanwhile been taken by a point with observations;
        such an item is redone alone against the current slots with the reference's expressions (_ff_one, raising
        what they raise).  An unmarked item without a candidate or above TH_HIGH is never redone.  Assignment, the
        count and the rotation histogram with its rejection follow the reference, including a feature that is
        assigned twice (a point without observations overwritten) being counted and rejected twice.  A pair takes
        the single call at its place when its th is not a plain finite number, when either mTcw is not a finite 4 x 4
        float32 / float64 array, when _ff_frame refuses the current frame, when a candidate's octave is not an int
        inside the current frame's scale table, or when mvpMapPoints is not a list of N entries.  The loop itself
        runs when a current frame, or its mvpMapPoints list, occurs twice or also serves as a last frame of the
        call, and where the HIP runtime sees no device.  A last frame may serve several pairs."""
        curs, lasts = list(current_frames), list(last_frames)
        if len(curs) != len(lasts):
            raise ValueError("one last frame per current frame")
        if isinstance(th, (list, tuple, np.ndarray)) and np.ndim(th) == 1:
            ths = list(th)
            if len(ths) != len(curs):
                raise ValueError("one th per pair, or one for all")
        else:
            ths = [th] * len(curs)
        res = [None] * len(curs)
        slots = lambda f: id(getattr(f, "mvpMapPoints", f))  # noqa: E731
        distinct = (len({id(c) for c in curs}) == len(curs) == len({slots(c) for c in curs})
                    and not {id(c) for c in curs} & {id(x) for x in lasts}
                    and not {slots(c) for c in curs} & {slots(x) for x in lasts})
        if curs and distinct and _lib.device_present():
            packed = [self._ff_job(c, x, t) for c, x, t in zip(curs, lasts, ths)]
            take = [k for k, j in enumerate(packed) if j is not None]
            if take:
                for k, n in zip(take, self._ff_jobs([(curs[k], lasts[k], ths[k], packed[k]) for k in take])):
                    res[k] = n
        return [self.search_by_projection_f_f(c, x, t) if r is None else r
                for c, x, t, r in zip(curs, lasts, ths, res)]

    def _fkf_host(self, CurrentFrame, pKF, sAlreadyFound, th, ORBdist):
        """search_by_projection_f_kf_f on the host, point by point (only the Hamming distances run on the device):
        the fallback of the public method."""
        Rcw = CurrentFrame.mTcw[:3, :3]
        tcw = CurrentFrame.mTcw[:3, 3:4]
        Ow = -np.dot(Rcw.T, tcw)
        rot_hist = [[] for _ in range(HISTO_LENGTH)]
        factor = 1.0 / HISTO_LENGTH
        work = []
        for i, pMP in enumerate(pKF.get_map_point_matches()):
            if not (pMP and not pMP.is_bad() and pMP not in sAlreadyFound):
                continue
            x3Dw = pMP.get_world_pos()
            x3Dc = np.dot(Rcw, x3Dw) + tcw
            invzc = 1.0 / x3Dc[2]
            u = CurrentFrame.fx * x3Dc[0] * invzc + CurrentFrame.cx
            v = CurrentFrame.fy * x3Dc[1] * invzc + CurrentFrame.cy
            if u < CurrentFrame.mnMinX or u > CurrentFrame.mnMaxX or v < CurrentFrame.mnMinY or v > CurrentFrame.mnMaxY:
                continue
            PO = x3Dw - Ow
            dist3D = np.linalg.norm(PO)
            maxDistance = pMP.get_max_distance_invariance()
            minDistance = pMP.get_min_distance_invariance()
            if dist3D < minDistance or dist3D > maxDistance:
                continue
            lvl = pMP.predict_scale(dist3D, CurrentFrame)
            vIndices2 = CurrentFrame.get_features_in_area(u, v, th * CurrentFrame.mvScaleFactors[lvl], lvl - 1, lvl + 1)
            if not vIndices2:
                continue
            work.append((i, pMP, vIndices2, pMP.get_descriptor()))
        n_matches = 0
        for (i, pMP, cands, _), dq in zip(work, self._batched([(w[3], w[2]) for w in work],
                                                             CurrentFrame.mDescriptors)):
            best_dist, best_idx2 = 256, -1
            for i2, dist in zip(cands, dq.tolist()):
                if CurrentFrame.mvpMapPoints[i2]:
                    continue
                if dist < best_dist:
                    best_dist = dist
                    best_idx2 = i2
            if best_dist <= ORBdist:
                CurrentFrame.mvpMapPoints[best_idx2] = pMP
                n_matches += 1
                if self.mbCheckOrientation:
                    rot = pKF.mvKeysUn[i].angle - CurrentFrame.mvKeysUn[best_idx2].angle
                    if rot < 0.0:
                        rot += 360.0
                    b = round(rot * factor)
                    if b == HISTO_LENGTH:
                        b = 0
                    assert 0 <= b < HISTO_LENGTH
                    rot_hist[b].append(best_idx2)
        if self.mbCheckOrientation:
            n_matches -= self._reject_by_rotation(rot_hist,
                                                  lambda i: CurrentFrame.mvpMapPoints.__setitem__(i, None))
        return n_matches
