"""Margin cases for k_ff_search, in the style of tests/margin_cases.py: per gate and precision a small world in the
non-dyadic camera of the matcher goldens (fx = 718.856, a 1241 x 376 image in 64 x 48 cells, a pose with a little
rotation), in which one coordinate of a map point is bisected over its dtype's values until the reference body's
decision flips between two neighbours; the rungs are the two neighbours and the values 2^j - 1 units in the last place
further out on either side (j = 0..12).  A decision is read off what the reference body (ff_oracle.ff_one, the
statements of ORBMatcher.py:314-367 on stand-in objects) returns: a candidate or none; for the depth gate, which both
sides leave without a candidate, off the sign of the reference's own 1 / pc.z.

Gates: |dx| and |dy| at the radius, the stereo gate at the radius, the four image bounds, an upper window end at a cell
border (a feature the grid stores one cell up is visited or not), and the sign of pc.z.

A set: name, gate, dtype, cur / last / th (one pair whose last frame holds one map point per rung), values (the rungs
in ascending distance from the flip, the found side first), found (the reference's decision per rung) and flip (the
two adjacent rungs).
"""
from __future__ import annotations

import numpy as np

import ff_cases as FC
import ff_oracle as FO
import matcher_frames as MF
from bow_match_cases import D
from conftest import BF, FX

J = 12
W, H = 1241, 376
CX, CY = 607.1928, 185.2157
WINV, HINV = 64.0 / W, 48.0 / H
GATES = ("dx", "dy", "stereo", "max_x", "min_x", "max_y", "min_y", "window", "depth")
PRECS = (np.float32, np.float64)


def _ordinal(x, dtype):
    """The position of x among its dtype's values, monotone in x."""
    it = np.int32 if dtype is np.float32 else np.int64
    o = int(np.array(x, dtype).view(it))
    return o if o >= 0 else int(np.iinfo(it).min) - o


def _value(o, dtype):
    it = np.int32 if dtype is np.float32 else np.int64
    if o < 0:
        o = int(np.iinfo(it).min) - o
    return dtype(np.array(o, it).view(dtype))


def _pose(dtype):
    a = np.array([0.013, -0.021, 0.017])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    U, _, Vt = np.linalg.svd(np.eye(3) + K + K @ K / 2)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = (U @ Vt).astype(dtype)
    T[:3, 3] = np.array([0.31, -0.17, 0.23]).astype(dtype)
    return T


def _world(T, u, v, z):
    """The world point that lands on (u, v) from depth z, in double."""
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    return R.T @ (np.array([(u - CX) * z / FX, (v - CY) * z / FX, z]) - t)


def _setup(gate):
    """(feature x, y, uR), th, the projections (u, v) of a point that is found and of one that is not, the coordinate
    that moves, and the depth."""
    z = 11.0
    cx3, cy3 = (30 + 0.2) / WINV, (23 + 0.2) / HINV          # stored in, and truncated to, cell (30, 23)
    if gate == "dx":
        return (cx3, cy3, -1.0), 7.0, (cx3 - 6.5, cy3 + 0.3), (cx3 - 7.5, cy3 + 0.3), 0, z
    if gate == "dy":
        return (cx3, cy3, -1.0), 7.0, (cx3 + 0.3, cy3 - 6.5), (cx3 + 0.3, cy3 - 7.5), 1, z
    if gate == "stereo":
        u = cx3 - 0.7
        return (cx3, cy3, u - BF / z + 6.5), 7.0, (u, cy3 + 0.3), (u - 1.0, cy3 + 0.3), 0, z
    if gate == "max_x":
        return ((63 + 0.2) / WINV, cy3, -1.0), 30.0, (W - 0.5, cy3), (W + 0.5, cy3), 0, z
    if gate == "min_x":
        return (0.2 / WINV, cy3, -1.0), 30.0, (0.5, cy3), (-0.5, cy3), 0, z
    if gate == "max_y":
        return (cx3, (47 + 0.2) / HINV, -1.0), 30.0, (cx3, H - 0.5), (cx3, H + 0.5), 1, z
    if gate == "min_y":
        return (cx3, 0.2 / HINV, -1.0), 30.0, (cx3, 0.5), (cx3, -0.5), 1, z
    if gate == "window":
        # the feature lies a quarter cell below the border of column 10 and is stored in column 10 (the grid rounds);
        # the window's upper end, (u + 7) / cell width, crosses 10
        kx, edge = (10 - 0.25) / WINV, 10 / WINV
        return (kx, cy3, -1.0), 7.0, (edge - 7.0 + 0.5, cy3), (edge - 7.0 - 0.5, cy3), 0, z
    raise KeyError(gate)


class Set:
    pass


def _frames(dtype, feat, points):
    a = dict(x=np.array([feat[0]], np.float32), y=np.array([feat[1]], np.float32), octave=np.zeros(1, np.int32),
             angle=np.zeros(1, np.float32), desc=D(9).reshape(1, 32), uR=np.array([feat[2]], np.float32))
    cur = FC.Frame(a, _pose(dtype))
    if feat[2] > 0:
        cur.mvuRight = [float(feat[2])]          # a double: the float32 list would move the gate by its own rounding
    cur.mvKeys[0].pt = (float(feat[0]), float(feat[1]))   # the exact doubles, not their float32 roundings
    cur._grid()
    n = len(points)
    b = dict(x=np.zeros(n, np.float32), y=np.zeros(n, np.float32), octave=np.zeros(n, np.int32),
             angle=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), uR=np.full(n, -1.0, np.float32))
    last = FC.Frame(b, _pose(dtype))
    last.mvpMapPoints = [MF.MP(D(), pos=p.reshape(3, 1), obs=1) for p in points]
    return cur, last


def _ref_invz_negative(cur, p):
    with np.errstate(all="ignore"):
        x3Dc = cur.mTcw[:3, :3] @ p.reshape(3, 1) + cur.mTcw[:3, 3:4]
        return bool(1.0 / x3Dc[2][0] < 0)


def build(gate, dtype):
    S = Set()
    S.name, S.gate, S.dtype = f"{gate}_{'f32' if dtype is np.float32 else 'f64'}", gate, dtype
    T = _pose(dtype)
    if gate == "depth":
        feat, S.th, axis = (600.0, 180.0, -1.0), 7.0, 2
        A, B = _world(T, 600.0, 180.0, 0.5).astype(dtype), _world(T, 600.0, 180.0, -0.5).astype(dtype)
        B[:2] = A[:2]
    else:
        feat, S.th, ua, ub, axis, z = _setup(gate)
        A, B = _world(T, *ua, z).astype(dtype), _world(T, *ub, z).astype(dtype)
        B[1 - axis], B[2] = A[1 - axis], A[2]
    probe_cur, probe_last = _frames(dtype, feat, [A])

    def decide(val):
        p = A.copy()
        p[axis] = val
        if gate == "depth":
            return not _ref_invz_negative(probe_cur, p)
        probe_last.mvpMapPoints[0]._p = p.reshape(3, 1)
        return FO.ff_one(probe_cur, probe_last, 0, probe_last.mvpMapPoints[0], S.th, 0)[1] >= 0
    lo, hi = _ordinal(A[axis], dtype), _ordinal(B[axis], dtype)
    assert decide(_value(lo, dtype)) and not decide(_value(hi, dtype)), S.name
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if decide(_value(mid, dtype)):
            lo = mid
        else:
            hi = mid
    step = 1 if lo < hi else -1
    ords = []
    for j in range(J + 1):
        ords += [lo - step * (2 ** j - 1), hi + step * (2 ** j - 1)]
    S.values = [_value(o, dtype) for o in ords]
    S.flip = (0, 1)
    pts = []
    for val in S.values:
        p = A.copy()
        p[axis] = val
        pts.append(p)
    S.found = [decide(v) for v in S.values]
    S.cur, S.last = _frames(dtype, feat, pts)
    return S


_SETS = {}


def get(gate, dtype):
    key = (gate, dtype)
    if key not in _SETS:
        _SETS[key] = build(gate, dtype)
    return _SETS[key]


def all_sets():
    return [get(g, d) for g in GATES for d in PRECS]


def arrays(S):
    """The entry's arrays of the set's pair: one search, one item per rung."""
    return FO.pack([(S.cur, S.last, S.th)])[0]


def reference(S):
    """(best_idx, best_dist) per rung by the reference body, -1 for none."""
    out = []
    for i, p in enumerate(S.last.mvpMapPoints):
        bd, bi = FO.ff_one(S.cur, S.last, i, p, S.th, 0)
        out.append((bi, bd if bi >= 0 else -1))
    return out


def oracle_depth_negative(a, i):
    K, P = a["kf_f64"][0], a["pt_f64"][int(a["item_pt"][i])]
    return float(((K[11] * P[0] + K[12] * P[1]) + K[13] * P[2]) + K[16]) < 0.0
